"""train_scripts/train.py from pictures, end to end on the GPU, one subprocess per mode under `timeout`:

  * pictures with caption feature files (load_vae_feat = False, load_t5_feat = True) at 256px, bf16 operands: 2 steps, finite loss, a checkpoint;
  * pictures with text captions (load_t5_feat = False) under mixed_precision = 'fp16', so that the T5 encoder runs in its bf16 worker process: the tokenizer is a
    tiny sentencepiece model trained on the test's captions on the CPU and loaded by transformers' AutoTokenizer, the T5 a one-block encoder of random weights
    at d_model 4096 (the width the denoiser's caption projection takes); real_prompt_ratio = 0.5 mixes the two caption kinds.

Data: 4 generated PNGs under <tmp>/InternImgs, data_info.json and the caption files under <tmp>/InternData (the reference's InternalDataSigma layout); the VAE
is random-init (no vae_pretrained directory), the denoiser PixArtMS_XL_2 at 256px, batch 2."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_refs as R
import t5_refs
from conftest import ROOT

pytestmark = pytest.mark.gpu

L = 16
CAPTIONS = ["a red cube on a table", "two blue spheres over a green field", "one dog and one cat", "a small house under a big tree"]
LONG = ["a long caption of a picture with a red cube and many small words in it", "a long caption of two blue spheres", "a long caption of one dog",
        "a long caption of a small house"]
CONFIG = """
data_root = {root!r}
image_list_json = ['data_info.json']
data = dict(type='InternalDataSigma', root='InternData', image_list_json=image_list_json, transform='default_train', load_vae_feat=False, load_t5_feat={t5_feat})
image_size = 256
model = 'PixArtMS_XL_2'
mixed_precision = {mp!r}
vae_pretrained = {root!r} + '/no_vae_here'
t5_path = {t5_path!r}
num_workers = 2
train_batch_size = 2
model_max_length = {L}
optimizer = dict(type='AdamW', lr=2e-5, weight_decay=3e-2, eps=1e-10)
log_interval = 1
save_model_steps = 2
scale_factor = 0.13025
real_prompt_ratio = {ratio}
"""


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    Image = pytest.importorskip("PIL.Image")
    top = tmp_path_factory.mktemp("train_pictures")
    root, imgs = top / "InternData", top / "InternImgs" / "pics"
    (root / "caption_features_new").mkdir(parents=True)
    imgs.mkdir(parents=True)
    meta, g = [], torch.Generator().manual_seed(0)
    for i, (h, w) in enumerate(((300, 280), (260, 400), (512, 512), (256, 257))):
        Image.fromarray(R.make_image(h, w, seed=i)).save(imgs / f"p{i}.png")
        meta.append({"path": f"pics/p{i}.png", "height": h, "width": w, "ratio": h / w, "prompt": CAPTIONS[i], "sharegpt4v": LONG[i]})
        np.savez(root / "caption_features_new" / f"p{i}.npz", caption_feature=torch.randn(1, 5 + i, 4096, generator=g).to(torch.float16).numpy(),
                 attention_mask=np.ones((1, 5 + i), dtype=np.int64))
    (root / "data_info.json").write_text(json.dumps(meta))
    return top


def _run(tree, tmp_path, **kw):
    cfg = tmp_path / "cfg.py"
    cfg.write_text(CONFIG.format(root=str(tree), L=L, **kw))
    env = {k: v for k, v in os.environ.items() if k not in ("PXA_OPERAND_DTYPE", "PXA_LIB_PATH")}
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_scripts", "train.py"), str(cfg), "--max-steps", "2",
                        "--work-dir", str(tmp_path / "w")], capture_output=True, text=True, cwd=ROOT, env=env)
    print("\n" + r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(lines) == 2
    for ln in lines:
        loss = float(ln.split("loss ")[1].split()[0])
        assert loss == loss and abs(loss) < 1e4, ln                                                  # finite
    ck = torch.load(tmp_path / "w" / "checkpoints" / "epoch_1_step_2.pth", map_location="cpu", weights_only=False)
    assert ck["step"] == 2 and all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    return r.stdout


def test_train_from_pictures_and_caption_files(tree, tmp_path):
    out = _run(tree, tmp_path, t5_feat=True, mp="bf16", t5_path="unused", ratio=1.0)
    assert "data: pictures of " + str(tree / "InternData") + " with caption feature files" in out and "operands bf16" in out


def test_train_from_pictures_and_text_under_fp16(tree, tmp_path):
    spm = pytest.importorskip("sentencepiece")
    from safetensors.torch import save_file
    t5 = tmp_path / "t5"
    t5.mkdir()
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter((CAPTIONS + LONG) * 4), model_writer=model, vocab_size=48, model_type="unigram", pad_id=0, eos_id=1,
                                   unk_id=2, bos_id=-1, hard_vocab_limit=False)
    (t5 / "spiece.model").write_bytes(model.getvalue())
    (t5 / "tokenizer_config.json").write_text(json.dumps({"tokenizer_class": "T5Tokenizer", "extra_ids": 0, "model_max_length": L}))
    cfg = dict(d_model=4096, num_heads=64, d_ff=256, num_layers=1, vocab_size=64)
    (t5 / "config.json").write_text(json.dumps(dict(t5_refs.full_config(cfg), model_type="t5")))
    save_file({k: v.clone() for k, v in t5_refs.state_dict(cfg, 31).items() if k != "encoder.embed_tokens.weight"}, str(t5 / "model.safetensors"))
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(str(t5))(CAPTIONS, max_length=L, padding="max_length", truncation=True, return_tensors="pt")
    assert int(tok["input_ids"].max()) < 64 and tok["attention_mask"].sum(1).min() >= 2             # the tiny tokenizer loads and its ids fit the vocabulary
    out = _run(tree, tmp_path, t5_feat=False, mp="fp16", t5_path=str(t5), ratio=0.5)
    assert "with text captions" in out and "operands fp16" in out
    left = subprocess.run(["pgrep", "-f", f"--t5-path {t5}"], capture_output=True, text=True).stdout.split()      # the worker's own command line
    assert left == [], f"caption worker(s) still alive: {left}"
