"""CaptionEncoder (pixart_sigma_amd/t5/captions.py): caption strings to the denoiser's caption features, in this process under the bf16-operand build and
through a bf16 worker process under the fp16 one.

The model: one T5 block at the widths of T5-XXL that matter to the kernels (d_model 4096, 64 heads of 64) with a small feed-forward (d_ff 256) and a
64-entry vocabulary; random bf16-representable weights from tests/t5_refs.state_dict, written to tmp_path as config.json + model.safetensors.  The tokenizer
is a fake callable with the transformers call signature: a word becomes an id in [2, 64), id 1 ends a caption, id 0 pads; an empty caption is one token.

bf16 build: CaptionEncoder.encode equals T5Embedder.get_text_embeddings on the same encoder bit for bit (ragged lengths, a one-token caption), and the host mask
is the tokenizer's.
f16 build: the worker path is taken; two workers started one after another agree bit for bit; the features meet the bound tests/test_t5_model_gpu.py uses,
1.1 x the yardstick of tests/golden/t5_ref_noise.json, against tests/t5_refs.encoder64 in fp64 - the bf16 yardstick, since the worker computes in bf16 (as
test_t5_model_gpu.test_feature_tool_end_to_end takes it), and the smaller of the file's two.
Both builds (worker=True forces the worker under bf16 too): the worker's features are the in-process features rounded to bf16, bit for bit (bf16 build, where
both exist); a worker given a time limit it cannot meet raises CaptionWorkerError in the parent, no child is left alive, and it is not restarted.
Every CaptionEncoder made here is closed by a finalizer, which terminates and reaps its worker.

The file runs again under the fp16-operand build in a child process."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import t5_fixtures
import t5_refs
from conftest import ROOT, record_parity, rel_l2

pytestmark = pytest.mark.gpu

CFG = dict(d_model=4096, num_heads=64, d_ff=256, num_layers=1, vocab_size=64)
SEED, L, MARGIN = 31, 24, 1.1
TEXTS = ["a red cube on a table", "", "two blue spheres", "one " * 40, "a"]          # ragged; '' is one token (the end marker); 'one ' * 40 is truncated to L


def fake_tokenizer(texts, max_length=None, padding=None, truncation=None, return_tensors=None, **kw):
    assert padding == "max_length" and truncation and return_tensors == "pt"
    ids = torch.zeros(len(texts), max_length, dtype=torch.int64)
    mask = torch.zeros(len(texts), max_length, dtype=torch.int64)
    for i, t in enumerate(texts):
        toks = [2 + sum(w.encode()) % 62 for w in t.split()][: max_length - 1] + [1]
        ids[i, :len(toks)] = torch.tensor(toks)
        mask[i, :len(toks)] = 1
    return {"input_ids": ids, "attention_mask": mask}


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safetensors.torch import save_file
    path = tmp_path_factory.mktemp("t5_one_block")
    sd = t5_refs.state_dict(CFG, SEED)
    with open(path / "config.json", "w") as f:
        json.dump(dict(t5_refs.full_config(CFG), model_type="t5"), f)
    save_file({k: v.clone() for k, v in sd.items() if k != "encoder.embed_tokens.weight"}, str(path / "model.safetensors"))
    return str(path), sd


@pytest.fixture
def make(request, model_dir):
    from pixart_sigma_amd.t5.captions import CaptionEncoder

    def build(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ce = CaptionEncoder(model_dir[0], fake_tokenizer, model_max_length=L, max_batch=8, **kw)
        request.addfinalizer(ce.close)
        return ce
    return build


@pytest.fixture(scope="module")
def reference(model_dir):
    tok = fake_tokenizer(TEXTS, max_length=L, padding="max_length", truncation=True, return_tensors="pt")
    want = t5_refs.encoder64(CFG, model_dir[1], tok["input_ids"], tok["attention_mask"], device="cuda")[-1]
    return tok, want


def _bound():
    noise = t5_fixtures.ref_noise()
    return MARGIN * min(noise["t5_tiny"]["bf16"], noise["t5_l300"]["bf16"])


def test_encode_by_build(make, reference):
    from pixart_sigma_amd import lib
    tok, want = reference
    ce = make()
    y, mask = ce.encode(TEXTS)
    assert y.dtype == torch.float32 and tuple(y.shape) == (len(TEXTS), 1, L, 4096) and y.is_cuda and torch.isfinite(y).all()
    assert mask.dtype == torch.int64 and not mask.is_cuda and torch.equal(mask, tok["attention_mask"])
    assert mask.sum(1).tolist() == [7, 1, 4, L, 2]
    err = rel_l2(y[:, 0], want)
    record_parity(f"caption features of the {lib.OPERAND} build's CaptionEncoder vs encoder64 (bound = {MARGIN} x transformers' own bf16 error)", err, _bound())
    print(f"\nCaptionEncoder [{lib.OPERAND} build, {'in process' if ce.in_process else 'worker'}]: rel-L2 {err:.3e} against encoder64 (bound {_bound():.3e})")
    assert err <= _bound()
    if lib.OPERAND == "bf16":
        from pixart_sigma_amd.t5 import T5Embedder
        assert ce.in_process and ce.worker is None
        embs, m = T5Embedder(ce.encoder, fake_tokenizer, model_max_length=L).get_text_embeddings(TEXTS)
        assert torch.equal(y[:, 0], embs) and torch.equal(mask, m.cpu())
        one, m1 = ce.encode([""])                                                                      # a one-token caption alone
        e1, m2 = T5Embedder(ce.encoder, fake_tokenizer, model_max_length=L).get_text_embeddings([""])
        assert m1.sum().item() == 1 and tuple(one.shape) == (1, 1, L, 4096) and torch.equal(one[:, 0], e1) and torch.equal(m1, m2.cpu())
    else:
        assert not ce.in_process and ce.worker is not None and ce.worker.alive                        # the worker path is taken
        ce.close()
        assert not ce.worker.alive


def test_two_workers_agree_and_a_missed_time_limit_raises(make):
    from pixart_sigma_amd import lib
    from pixart_sigma_amd.t5.captions import CaptionWorkerError
    a = make(worker=True)
    ya, ma = a.encode(TEXTS)
    pid_a = a.worker.proc.pid
    a.close()
    assert not a.worker.alive
    b = make(worker=True)
    assert b.worker.alive and b.worker.proc.pid != pid_a
    yb, mb = b.encode(TEXTS)
    assert torch.equal(ya, yb) and torch.equal(ma, mb)
    first = b.submit(TEXTS[:2])                                                                       # two requests in flight, collected in order
    second = b.submit(TEXTS[2:])
    y1, y2 = b.collect(), b.collect()
    assert torch.equal(torch.cat([first, second]), mb) and b.outstanding == 0
    assert torch.equal(y1, b.encode(TEXTS[:2])[0]) and torch.equal(y2, b.encode(TEXTS[2:])[0])
    assert tuple(y1.shape) == (2, 1, L, 4096) and tuple(y2.shape) == (3, 1, L, 4096)
    if lib.OPERAND == "bf16":                                                                          # what crosses the shared block is the in-process result as bf16
        y, _ = make().encode(TEXTS)
        assert torch.equal(yb, y.to(torch.bfloat16).float())
    # a time limit the worker cannot meet: the parent raises with the worker's stderr tail, the child is gone and stays gone
    b.worker.timeout = 1e-6
    with pytest.raises(CaptionWorkerError, match="time limit") as info:
        b.encode(TEXTS)
    assert "not restarted" in str(info.value) and "stderr ends" in str(info.value)
    assert not b.worker.alive and b.worker.proc.returncode is not None
    with pytest.raises(CaptionWorkerError, match="time limit"):
        b.encode(TEXTS)
    assert not b.worker.alive


def test_f16_build_runs_this_file():
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln or "CaptionEncoder [" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
