"""fp32 outputs of the persistent TN (weight-gradient) GEMM on fixed seeded inputs, saved to a file: two libraries (PXA_LIB_PATH) must produce the same bits
(tests/test_gemm_tn_m16_gpu.py: the product library against its -DGEMM_WAIT_ALL=1 build).  Shapes: 6 k-units per item (two steady-state units, then the
drain), the paired remainder column with a padded last pair at 10 units, and four ragged k-slices into slabs.   usage: python tools/gemm_tn_dump.py OUT.pt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pixart_sigma_amd import ops  # noqa: E402

SHAPES = [(1024, 1024, 192, 1), (2304, 1152, 320, 1), (1152, 1152, 960, 4)]      # (M, N, K, split_k)


def main(out_path):
    res = {}
    for M, N, K, split_k in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + K)
        a = torch.randn(K, M, generator=g, device="cuda").to(ops.BF16)
        b = torch.randn(K, N, generator=g, device="cuda").to(ops.BF16)
        assert ops.gemm_plan(a, b, ops.TN, out_f32=torch.empty(M, N, device="cuda"), accumulate=True, split_k=split_k).startswith("gemm_pers_kernel<2,")
        out = torch.zeros(M, N, device="cuda")
        for _ in range(2):
            ops.gemm(a, b, ops.TN, out_f32=out, accumulate=True, split_k=split_k)
        res[f"tn_{M}x{N}_k{K}_s{split_k}"] = out.cpu()
    torch.cuda.synchronize()
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
