"""CPU checks of the denoiser's MXFP8 inference path (csrc/gemm_f8.hip): the host reference's own properties (tests/mx_fp8_refs.py), every refusal of
pxa_gemm_f8_plan with its message, the plan line, the ctypes struct against the header, the emitted ISA (no scratch, the block-scaled MFMA), and the
engine's FP8 schedule through a stand-in for pixart_sigma_amd.ops.  No GPU."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mx_fp8_refs as R  # noqa: E402

FP8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------ the reference's own properties
def _wide_magnitudes(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.empty(rows, K // 32, 1).uniform_(-20, 14, generator=g)).expand(rows, K // 32, 32).reshape(rows, K)
    return torch.randn(rows, K, generator=g) * mag


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_never_clips(dtype):
    x = _wide_magnitudes(64, 256, 0).to(dtype)
    if dtype == torch.float16:
        x = x.clamp(-6e4, 6e4)
    X = R.exponents(x)
    y = x.double().abs().reshape(64, 8, 32).amax(dim=2) / torch.exp2(X.double())
    assert (y <= 448.0).all(), "a block maximum lands above 448: the conversion would clip"
    nz = y > 0
    assert (y[nz] > 224.0).all(), "a block maximum lands at or below 224: the exponent is one too large"
    q, e = R.quant_rows(x)
    bits = q.view(torch.uint8)
    assert not ((bits & 0x7F) == 0x7F).any(), "an e4m3fn NaN code was written"
    assert (e != 0xFF).all(), "the E8M0 NaN code was written"
    # elements that land in e4m3's normal range (|x / 2^X| >= 2^-6): relative error at most 2^-4
    y = x.double() / torch.exp2(X.double()).repeat_interleave(32, dim=1)
    n = y.abs() >= 2.0 ** -6
    rel = ((q.double() - y).abs() / y.abs().clamp_min(1e-300))[n]
    assert rel.max() <= 2.0 ** -4, rel.max()


def test_reference_edges():
    x = torch.zeros(3, 64)
    x[1, :32] = 448.0 * 2.0 ** -5                   # amax exactly 448 * 2^k: X = k, the maximum lands on 448
    x[1, 32:] = 448.0 * 2.0 ** -5 * (1 + 2.0 ** -23)  # one fp32 ulp above: X = k + 1
    x[2, 0] = 1e-45                                  # an fp32 subnormal: the lower clamp
    x[2, 32] = 3e38                                  # near the top of fp32
    q, e = R.quant_rows(x)
    assert e[0].tolist() == [127, 127] and (q[0].float() == 0).all(), "a zero block gives byte 127 and zero codes"
    assert e[1].tolist() == [127 - 5, 127 - 4]
    assert q[1, 0].float() == 448.0 and q[1, 32].float() == 224.0
    assert e[2, 0] == 0 and e[2, 1] == 127 + 120 and q[2, 32].float().abs() <= 448


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_reference_round_trip_is_exact_on_the_grid(dtype):
    g = torch.Generator().manual_seed(1)
    q0 = torch.randint(0, 256, (32, 128), generator=g, dtype=torch.uint8)
    q0[(q0 & 0x7F) == 0x7F] = 0x38
    q0[:, ::32] = 0x7E                               # every block holds 448: the quantiser finds the block's exponent again
    e0 = torch.randint(127 - 10, 127 + 7, (32, 4), generator=g, dtype=torch.uint8)
    x = R.dequant(q0.view(FP8), e0, dtype)
    assert (x.double() == R.dequant(q0.view(FP8), e0)).all(), f"q * 2^(e - 127) is not exact in {dtype}"
    q1, e1 = R.quant_rows(x)
    assert (e1 == e0).all()
    assert (q1.float() == q0.view(FP8).float()).all()


def test_code_table_matches_torch():
    b = R.finite_codes()
    assert b.numel() == 254 and 0x80 in b.tolist() and 0x7F not in b.tolist() and 0xFF not in b.tolist()
    assert (R.code_values(b) == b.view(FP8).double()).all()
    assert R.code_values(torch.tensor([0x01, 0x7E, 0xFE], dtype=torch.uint8)).tolist() == [2.0 ** -9, 448.0, -448.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_rounds_ties_to_even(dtype):
    mid, want = R.tie_midpoints()
    assert mid.numel() == 252 and ((want & 1) == 0).all() and mid[0] == 2.0 ** -10 and mid[125] == 432.0
    x, q_want, e_want = R.tie_rows()
    assert (x.to(dtype).double() == x.double()).all(), f"a midpoint is not exact in {dtype}"
    for m, w in zip(mid.tolist(), want.tolist()):                # every midpoint is in every row, at its expected code
        hit = x[0] == m
        assert hit.sum() == 1 and q_want[0][hit].item() == w
    q, e = R.quant_rows(x.to(dtype))
    assert (e == e_want).all()
    bad = q.view(torch.uint8) != q_want
    assert not bad.any(), f"{bad.sum().item()} ties do not go to the even code; first {x[bad][0].item()} -> {q.view(torch.uint8)[bad][0].item():#x}"


def test_reference_exponent_edges_by_hand():
    x, X = R.exponent_edge_rows()
    assert (R.exponents(x) == X[:, None]).all(), (R.exponents(x)[:, 0] - X).tolist()
    q, e = R.quant_rows(x)
    assert (e.long() == X[:, None] + 127).all() and e.min() == 0
    assert not ((q.view(torch.uint8) & 0x7F) == 0x7F).any()
    at = (q[:, 5].float().abs(), q[:, 52].float().abs())
    assert ((at[0] >= 224) | (X == -127)).all() and (at[0] <= 448).all() and (at[0] == at[1]).all()


# ------------------------------------------------------------------------------------------------ the library's plan entry
def _operands(M, N, K):
    return (torch.zeros(M, K, dtype=torch.uint8).view(FP8), torch.zeros(M, K // 32, dtype=torch.uint8),
            torch.zeros(N, K, dtype=torch.uint8).view(FP8), torch.zeros(N, K // 32, dtype=torch.uint8))


@pytest.mark.parametrize("M", [1, 129, 16384])
def test_plan_line(M):
    from pixart_sigma_amd import ops
    qa, ea, qw, ew = _operands(M, 1152, 1152)
    line = ops.gemm_f8_plan(qa, ea, qw, ew, bias=torch.zeros(1152), act=ops.ACT_GELU, mx=True)
    mt = (M + 127) // 128
    assert line == f"gemm_f8_kernel<1,1,1> mfma=scale_16x16x128_f8f6f4 split=1 bm=128 bn=128 bk=128 m_tiles={mt} n_tiles=9 grid={9 * 8 * ((mt + 7) // 8)}", line
    assert ops.gemm_f8_plan(qa, ea, qw, ew).startswith("gemm_f8_kernel<0,1,0> ")
    assert ops.gemm_f8_plan(qa, ea, qw, ew, out16=False, mx=True).startswith("gemm_f8_kernel<0,0,1> ")


def test_plan_refusals():
    from pixart_sigma_amd import lib, ops
    with pytest.raises(lib.PixartHipError, match=r"N=64 must be a positive multiple of 128"):
        ops.gemm_f8_plan(*_operands(16, 64, 128))
    with pytest.raises(lib.PixartHipError, match=r"K=96 must be a positive multiple of 128"):
        ops.gemm_f8_plan(*_operands(16, 128, 96))
    qa, ea, qw, ew = _operands(16, 128, 128)
    flat = torch.zeros(16 * 128 + 16, dtype=torch.uint8)
    with pytest.raises(lib.PixartHipError, match=r"qa and qw must be 16-byte aligned"):
        ops.gemm_f8_plan(flat[1:1 + 16 * 128].view(16, 128).view(FP8), ea, qw, ew)
    with pytest.raises(lib.PixartHipError, match=r"out16 must be 16-byte aligned"):
        ops.gemm_f8_plan(qa, ea, qw, ew, out=torch.zeros(16 * 128 + 8, dtype=ops.BF16)[1:1 + 16 * 128].view(16, 128))
    with pytest.raises(lib.PixartHipError, match=r"no output: at least one of out16 and out_q / out_e must be given"):
        ops.gemm_f8_plan(qa, ea, qw, ew, out16=False)
    with pytest.raises(lib.PixartHipError, match=r"act=4 is not built"):
        ops.gemm_f8_plan(qa, ea, qw, ew, act=4)
    # a pitch that is no multiple of 16 bytes
    wide = torch.zeros(16, 136, dtype=torch.uint8).view(FP8)
    with pytest.raises(lib.PixartHipError, match=r"ldqa=136, ldqw=128 must be >= K and multiples of 16"):
        ops.gemm_f8_plan(wide[:, :128], ea, qw, ew)


def test_ctypes_struct_matches_header():
    from pixart_sigma_amd import lib
    src = open(os.path.join(ROOT, "include", "pixart_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pxa_gemm_f8_args", src, flags=re.S).group(1)
    fields, types_ = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = "p" if "*" in decl else decl.split()[0]
        for part in decl.split(","):
            fields.append(re.findall(r"[A-Za-z_0-9]+", part)[-1])
            types_.append(ctype)
    assert fields == [f[0] for f in lib.GemmF8Args._fields_]
    want = {"p": lib.c_void_p, "long": lib.c_long, "int": lib.c_int}
    assert [want[t] for t in types_] == [f[1] for f in lib.GemmF8Args._fields_]
    assert lib.SIGNATURES["pxa_gemm_f8"][0]._type_ is lib.GemmF8Args


# ------------------------------------------------------------------------------------------------ the emitted ISA
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from pixart_sigma_amd import build as B
    td = tmp_path_factory.mktemp("isa_f8")
    out = {}
    for tag, extra in (("bf16", []), ("f16", ["-DPXA_OPERAND_F16"])):
        o = str(td / f"gemm_f8.{tag}.s")
        subprocess.run([B._hipcc(), *B.FLAGS, *extra, "-I", B.INCLUDE, "-S", "--cuda-device-only", os.path.join(B.CSRC, "gemm_f8.hip"), "-o", o],
                       check=True, capture_output=True)
        out[tag] = open(o).read()
    return out


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_isa_no_scratch_and_scaled_mfma(asm, tag):
    text = asm[tag]
    kernels = re.findall(r"^\s*\.name:\s+(\S*_kernel\S*)\s*$", text, re.M)
    sizes = re.findall(r"^\s*\.private_segment_fixed_size:\s+(\d+)", text, re.M)
    assert len(kernels) == len(sizes) == 9, (kernels, sizes)      # 6 GEMM instances, 2 quantisers, 1 dequantiser
    assert all(s == "0" for s in sizes), dict(zip(kernels, sizes))
    assert "scratch_" not in text
    for name in kernels:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        n = len(re.findall(r"v_mfma_scale_f32_16x16x128_f8f6f4", body))
        assert n == (16 if "gemm_f8_kernel" in name else 0), (name, n)


# ------------------------------------------------------------------------------------------------ the engine's FP8 schedule
def _fake_ops(calls):
    import fake_ops
    ns = types.SimpleNamespace(**{k: v for k, v in vars(fake_ops).items() if not k.startswith("__")})
    real_gemm = ns.gemm

    def gemm(a, b, layout=fake_ops.NT, **kw):
        calls.append(("gemm", tuple(a.shape), tuple(b.shape)))
        return real_gemm(a, b, layout, **kw)

    def mx_quant_rows(x, q=None, e=None):
        calls.append(("mx_quant_rows", tuple(x.shape), q is not None))
        R_, K = x.shape
        return (q if q is not None else torch.zeros(R_, K, dtype=torch.uint8).view(FP8)), (e if e is not None else torch.zeros(R_, K // 32, dtype=torch.uint8))

    def mx_dequant_rows(q, e, out=None):
        calls.append(("mx_dequant_rows", tuple(q.shape)))
        return torch.zeros(q.shape, dtype=fake_ops.BF16)

    def gemm_f8(qa, ea, qw, ew, bias=None, act=0, out=None, out_q=None, out_e=None, out16=True, mx=False):
        M, N = qa.shape[0], qw.shape[0]
        assert qa.dtype == FP8 and qw.dtype == FP8 and tuple(ea.shape) == (M, qa.shape[1] // 32) and tuple(ew.shape) == (N, qw.shape[1] // 32)
        calls.append(("gemm_f8", M, N, qa.shape[1], act, bias is not None, out16, mx))
        o16 = torch.zeros(M, N, dtype=fake_ops.BF16) if out16 else None
        oq = (torch.zeros(M, N, dtype=torch.uint8).view(FP8), torch.zeros(M, N // 32, dtype=torch.uint8)) if mx else None
        return o16 if oq is None else (oq if o16 is None else (o16, *oq))
    ns.gemm, ns.mx_quant_rows, ns.mx_dequant_rows, ns.gemm_f8 = gemm, mx_quant_rows, mx_dequant_rows, gemm_f8
    return ns


@pytest.fixture
def fake_engine():
    from pixart_sigma_amd import engine
    from pixart_sigma_amd.model.nets.PixArtMS import PixArtMS
    calls = []
    keep = engine.ops
    engine.ops = _fake_ops(calls)
    try:
        torch.manual_seed(0)
        m = PixArtMS(depth=2, input_size=8, model_max_length=8, class_dropout_prob=0.0)
        m._prepare(torch.device("cpu"))
        yield m, calls
    finally:
        engine.ops = keep


def _forward(eng, save=None):
    B, L, D = 2, 8, 1152
    lens = [8, 5]
    row_idx = torch.tensor([b * L + i for b, n in enumerate(lens) for i in range(n)], dtype=torch.int32)
    return eng.forward(torch.zeros(B, 4, 8, 8), torch.zeros(B * L, 4096), torch.zeros(2, B, 6, D), torch.zeros(B, 2, D), row_idx, lens, None, save)


@pytest.mark.parametrize("mode", ["mx", "dequant"])
def test_fp8_forward_schedule(fake_engine, mode):
    m, calls = fake_engine
    eng, D, M = m._engine, 1152, 2 * 16
    m.enable_fp8(mode)
    assert m.fp8 == mode and eng.fp8 == mode
    # the weight copies: attn.qkv of both blocks in one launch from the prescaled copy, the other five per block, all into the engine's own buffers
    wq = [c for c in calls if c[0] == "mx_quant_rows"]
    assert len(wq) == 1 + 5 * 2 and all(c[2] for c in wq) and wq[0][1] == (2 * 3 * D, D)
    addrs = {n: (q.data_ptr(), e.data_ptr()) for n, (q, e) in eng._f8.items()}
    del calls[:]
    with torch.no_grad():
        _forward(eng)
    six = {(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)}
    token_gemms = [c for c in calls if c[0] == "gemm" and c[1][0] == M and c[2] in six]
    f8 = [c for c in calls if c[0] == "gemm_f8"]
    if mode == "mx":
        assert len(f8) == 6 * 2 and not token_gemms
        per_block = [(M, 3 * D, D, 0, True, True, False), (M, D, D, 0, True, True, False), (M, D, D, 0, True, True, False), (M, D, D, 0, True, True, False),
                     (M, 4 * D, D, 1, True, False, True), (M, D, 4 * D, 0, True, True, False)]
        assert [c[1:] for c in f8] == per_block * 2
        assert sum(c[0] == "mx_quant_rows" for c in calls) == 5 * 2          # xn1, a, x1b, cr, xn2; h leaves fc1 quantised
        assert not any(c[0] == "mx_dequant_rows" for c in calls)
    else:
        assert not f8 and len(token_gemms) == 6 * 2
        assert sum(c[0] == "mx_quant_rows" for c in calls) == 6 * 2 and sum(c[0] == "mx_dequant_rows" for c in calls) == 12 * 2
    # a weight change re-quantises in place
    del calls[:]
    m._store.bump()
    assert sum(c[0] == "mx_quant_rows" for c in calls) == 11
    assert addrs == {n: (q.data_ptr(), e.data_ptr()) for n, (q, e) in eng._f8.items()}
    # off: no FP8 call is left, and a bump no longer touches the copies
    m.disable_fp8()
    assert m.fp8 is None
    del calls[:]
    m._store.bump()
    with torch.no_grad():
        _forward(eng)
    assert not any(c[0] in ("gemm_f8", "mx_quant_rows", "mx_dequant_rows") for c in calls)
    assert len([c for c in calls if c[0] == "gemm" and c[1][0] == M and c[2] in six]) == 6 * 2


def test_fp8_refuses_training_and_adapters(fake_engine):
    m, calls = fake_engine
    m.enable_fp8("mx")
    with pytest.raises(RuntimeError, match="torch.no_grad"):
        _forward(m._engine, save="all")
    with pytest.raises(RuntimeError, match="torch.no_grad"):
        _forward(m._engine)                           # gradients enabled
    with pytest.raises(RuntimeError, match="merge_and_unload"):
        m.add_lora(r=4)
    with pytest.raises(ValueError):
        m.enable_fp8("int8")
    m.disable_fp8()
    m._lora = object()                                # stands for attached adapters
    try:
        with pytest.raises(RuntimeError, match=r"merge_and_unload\(\) first"):
            m.enable_fp8("mx")
    finally:
        m._lora = None
    assert m.fp8 is None
