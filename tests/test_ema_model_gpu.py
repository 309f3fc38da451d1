"""WeightEMA, its swapped() context and ValidationSampler on a depth-2 PixArtMS (input_size 8, 8 text tokens, every parameter drawn N(0, 0.02) so that
no layer is zero) with a default AutoencoderKL, and the two training scripts as child processes.

EMA bound: 3 x (2^-23 max(|e|, |p|)) per element against the fp64 recurrence over the three observed masters - one pxa_ema_update bound
(tests/test_ema_kernels_gpu.py) per step; an earlier step's error only shrinks (x decay) in the later ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DECAY = 0.9          # >= 0.5: 1 - decay is exact in fp32
L = 8


def tiny_model(seed=0, train=True):
    from pixart_sigma_amd import PixArtMS
    m = PixArtMS(depth=2, input_size=8, model_max_length=L, class_dropout_prob=0.0)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = m.cuda().train(train)
    m.prepare("cuda")
    return m


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def inputs(B=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, 8, 8, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda(), torch.randn(B, 1, L, 4096, generator=g).cuda(),
            torch.tensor([[1] * L, [1] * 5 + [0] * (L - 5)][:B]))


def forward(m):
    x, t, y, mask = inputs()
    was = m.training
    m.eval()
    try:
        with torch.no_grad():
            return m(x, t, y, mask=mask)
    finally:
        m.train(was)


# ---------------------------------------------------------------------------------------------- 1. the EMA over optimizer steps
def run_steps(model, opt, ema, store, scaler=None, inf_at=None):
    """Three steps on random gradients, ema.update() behind each; returns the fp64 recurrence's value and the bound's scale max(|e_0|, |m_k|)."""
    g = torch.Generator(device="cuda").manual_seed(1)
    e = store.master.double().clone()
    scale_of_bound = store.master.abs().double()
    assert torch.equal(ema.ema, store.master) and ema.ema.data_ptr() != store.master.data_ptr() and ema.ema.numel() == store.total
    d = np.float64(np.float32(DECAY))
    for k in range(3):
        gr = torch.randn(store.total, device="cuda", generator=g) * 1e-3
        store.grad.copy_(gr * (scaler.value if scaler else 1.0))
        if k == inf_at:
            store.grad[123] = float("inf")
        before = bits(store.master), bits(ema.ema)
        opt.step()
        ema.update()
        if k == inf_at:                                        # the skipped step moves neither weights nor EMA
            assert scaler.found_inf and torch.equal(bits(store.master), before[0]) and torch.equal(bits(ema.ema), before[1])
            continue
        assert not torch.equal(bits(store.master), before[0])
        m = store.master.double()
        e = e + (1.0 - d) * (m - e)
        scale_of_bound = torch.maximum(scale_of_bound, m.abs())
    return e, scale_of_bound


def check_ema(ema, ref, scale_of_bound):
    err = (ema.ema.double() - ref).abs()
    bound = 3 * 2.0 ** -23 * scale_of_bound
    print(f"EMA vs fp64 recurrence: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond 3 x 2^-23 max(|e|, |p|)"
    assert not torch.equal(ema.ema, ema.store.master)


@pytest.mark.parametrize("kind", ["adamw", "adamw_scaler_inf", "came", "adapters"])
def test_ema_follows_the_optimizer(kind):
    from pixart_sigma_amd.dp import FusedAdamW, FusedCAME, LossScaler
    from pixart_sigma_amd.ema import WeightEMA
    m = tiny_model()
    scaler = LossScaler("cuda", init_scale=1024.0) if kind == "adamw_scaler_inf" else None
    base = bits(m._store.master)
    if kind == "adapters":
        m.add_lora(r=4, init_lora_weights=False)
        m.prepare("cuda")
    opt = FusedCAME(m, lr=1e-3) if kind == "came" else FusedAdamW(m, lr=1e-3, weight_decay=3e-2, scaler=scaler)
    ema = WeightEMA(m, DECAY, scaler=scaler)
    assert ema.store is opt.store
    if kind == "adapters":
        assert ema.store is m._lora.store and ema.ema.numel() == m._lora.store.total != m._store.total
    ref, sb = run_steps(m, opt, ema, ema.store, scaler, inf_at=1 if scaler else None)
    check_ema(ema, ref, sb)
    if kind == "adapters":
        assert torch.equal(bits(m._store.master), base)         # the frozen base is neither trained nor averaged


def test_update_raises_after_the_store_was_rebuilt():
    from pixart_sigma_amd.ema import WeightEMA
    m = tiny_model()
    ema = WeightEMA(m, DECAY)
    m._store = None
    m.prepare("cuda")
    with pytest.raises(RuntimeError, match="rebuilt its flat parameter store"):
        ema.update()


# ---------------------------------------------------------------------------------------------- 2. swapped()
def moved_ema(m, lora=False):
    """An EMA that differs from the live weights: one update after the master was perturbed."""
    from pixart_sigma_amd.ema import WeightEMA
    ema = WeightEMA(m, DECAY)
    st = ema.store
    g = torch.Generator(device="cuda").manual_seed(9)
    st.master.add_(torch.randn(st.total, device="cuda", generator=g) * 5e-3)
    st.refresh_shadow(force=True)
    ema.update()
    ema.ema.add_(torch.randn(st.total, device="cuda", generator=g) * 5e-3)
    return ema


def state_of(m, ema):
    st = ema.store
    return [bits(st.master), bits(ema.ema), bits(st.shadow), bits(m._store.shadow), bits(m._store.master)]


def test_swapped_runs_the_ema_weights_and_restores_every_bit():
    m = tiny_model(train=False)
    ema = moved_ema(m)
    live = forward(m)
    other = tiny_model(seed=5, train=False)
    other.load_state_dict({k: v.clone() for k, v in ema.state_dict().items()})
    want = forward(other)
    before, ptrs = state_of(m, ema), [p.data_ptr() for p in m.parameters()]
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    with ema.swapped():
        inside = forward(m)
        with pytest.raises(RuntimeError, match="does not nest"):
            with ema.swapped():
                pass
        with pytest.raises(RuntimeError, match="inside swapped"):
            ema.update()
    assert torch.equal(inside, want) and not torch.equal(inside, live)
    assert all(torch.equal(a, b) for a, b in zip(before, state_of(m, ema)))
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    del inside
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= mem + 4 * 1024 * 1024 < mem + 4 * ema.store.total       # no full-size temporary stays
    assert torch.equal(forward(m), live)
    # an exception inside still restores everything
    with pytest.raises(ZeroDivisionError):
        with ema.swapped():
            1 / 0
    assert all(torch.equal(a, b) for a, b in zip(before, state_of(m, ema)))
    assert torch.equal(forward(m), live)
    with ema.swapped():                                                                              # and the context is usable again
        assert torch.equal(forward(m), want)


def test_swapped_on_adapters_remerges():
    m = tiny_model(train=False)
    m.add_lora(r=4, init_lora_weights=False)
    m.prepare("cuda")
    ema = moved_ema(m)
    assert ema.on_adapters
    live = forward(m)
    other = tiny_model(train=False)
    lo = other.add_lora(r=4, init_lora_weights=False)
    with torch.no_grad():
        for n, v in ema.state_dict().items():
            lo.params[n].copy_(v)
    other.prepare("cuda")
    want = forward(other)
    before, ptrs = state_of(m, ema), [p.data_ptr() for p in m.lora_parameters()]
    with ema.swapped():
        inside = forward(m)
    assert torch.equal(inside, want) and not torch.equal(inside, live)
    assert all(torch.equal(a, b) for a, b in zip(before, state_of(m, ema)))
    assert ptrs == [p.data_ptr() for p in m.lora_parameters()]
    assert torch.equal(forward(m), live)


def test_a_captured_sampling_graph_survives_swapped():
    from pixart_sigma_amd import DPMS
    m = tiny_model(train=False)
    ema = moved_ema(m)
    x, _, y, mask = inputs()
    null = torch.randn(1, 1, L, 4096, generator=torch.Generator().manual_seed(4)).repeat(2, 1, 1, 1).cuda()
    solver = DPMS(m.forward_with_dpmsolver, condition=y, uncondition=null, cfg_scale=4.5, model_kwargs=dict(data_info=None, mask=mask))
    kw = dict(steps=3, order=2, skip_type="time_uniform", method="multistep")
    g1 = solver.sample_graphed(x, **kw).clone()
    graph = solver._graph
    with ema.swapped():
        inside = solver.sample(x, **kw)
    g2 = solver.sample_graphed(x, **kw)
    assert solver._graph is graph
    assert torch.equal(g2, g1) and not torch.equal(inside, g1)


# ---------------------------------------------------------------------------------------------- 3. ValidationSampler.run
@pytest.fixture(scope="module")
def vae():
    from pixart_sigma_amd.vae import AutoencoderKL
    torch.manual_seed(2)
    return AutoencoderKL().cuda()


def prompts_feats():
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(2, 1, L, 4096, generator=g).cuda()
    masks = torch.tensor([[1] * L, [1] * 3 + [0] * (L - 3)])
    return feats, masks, torch.randn(1, 1, L, 4096, generator=g).cuda()


@pytest.mark.parametrize("with_ema", [False, True])
def test_validation_run_contract(vae, tmp_path, with_ema):
    from PIL import Image
    from pixart_sigma_amd import DPMS, IDDPM
    from pixart_sigma_amd.dp import FusedAdamW, LossScaler
    from pixart_sigma_amd.validation import ValidationSampler
    m = tiny_model()
    scaler = LossScaler("cuda", init_scale=256.0)
    opt = FusedAdamW(m, lr=1e-3, scaler=scaler)
    ema = moved_ema(m)
    st = m._store
    st.grad.normal_(std=1e-3)
    opt.m.normal_(std=1e-3)
    opt.v.uniform_(0, 1e-3)
    feats, masks, null = prompts_feats()
    vs = ValidationSampler(m, vae, feats, masks, null, image_size=64, out_dir=str(tmp_path / "validation"), steps=3, seed=7)

    def contract():
        return [bits(st.master), bits(st.shadow), bits(st.grad), bits(opt.m), bits(opt.v), bits(ema.ema), bits(scaler.state), torch.get_rng_state(),
                torch.cuda.get_rng_state(), torch.tensor(m.training)]
    before, ptrs = contract(), [p.data_ptr() for p in m.parameters()]
    assert m.training
    latents = vs.run(5, ema=ema if with_ema else None)
    assert all(torch.equal(a, b) for a, b in zip(before, contract()))
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    # the same latents as direct DPMS calls on a second model with the same (or the EMA's) weights and the same noise
    other = tiny_model(seed=5, train=False)
    other.load_state_dict({k: v.clone() for k, v in (ema.state_dict() if with_ema else m.state_dict()).items()})
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator(device="cuda").manual_seed(7), device="cuda")
    hw, ar = torch.tensor([[64.0, 64.0]], device="cuda"), torch.tensor([[1.0]], device="cuda")
    d = tmp_path / "validation" / ("step_5_ema" if with_ema else "step_5")
    assert sorted(os.listdir(d)) == ["0.png", "1.png"] and len(latents) == 2
    for i in range(2):
        with torch.no_grad():
            want = DPMS(other.forward_with_dpmsolver, condition=feats[i:i + 1], uncondition=null, cfg_scale=4.5,
                        model_kwargs=dict(data_info={"img_hw": hw, "aspect_ratio": ar}, mask=masks[i:i + 1])).sample(
                            z.clone(), steps=3, order=2, skip_type="time_uniform", method="multistep")
            assert torch.equal(latents[i], want) and bool(torch.isfinite(want).all())
            x = vae.decode(latents[i].to(vae.dtype) / vae.config.scaling_factor).sample.float()
        img = torch.clamp(127.5 * x + 128.0, 0, 255).permute(0, 2, 3, 1).to("cpu", dtype=torch.uint8).numpy()[0]
        assert img.shape == (64, 64, 3) and np.array_equal(np.asarray(Image.open(d / f"{i}.png")), img)
    assert not torch.equal(latents[0], latents[1])
    # a second call: the same noise, hence the same latents
    again = vs.run(6, ema=ema if with_ema else None)
    assert all(torch.equal(a, b) for a, b in zip(latents, again))
    # a training step right behind it
    x0, t, y, mask = inputs()
    opt.zero_grad()
    loss = IDDPM("1000", learn_sigma=True, pred_sigma=True).training_losses(m, x0, t, model_kwargs=dict(y=y, mask=mask, data_info=None))["loss"].mean()
    scaler.scale(loss).backward()
    opt.step()
    ema.update()
    assert bool(torch.isfinite(loss)) and not scaler.found_inf and not torch.equal(bits(st.master), before[0])


# ---------------------------------------------------------------------------------------------- 4. the training scripts
def write_feats(d, n):
    os.makedirs(d, exist_ok=True)
    g = np.random.default_rng(0)
    for name in [str(i) for i in range(n)] + ["null"]:
        np.savez(os.path.join(d, name + ".npz"), caption_feature=g.standard_normal((1, 16, 4096)).astype(np.float32), attention_mask=np.ones((1, 16), dtype=np.int64))


CFG = ("image_size = 256\ntrain_batch_size = 2\nmodel_max_length = 16\nlog_interval = 1\nsave_model_steps = 2\nema_rate = 0.5\neval_sampling_steps = 100\n"
       "validation_prompts = ['dog', 'a red cube']\nvisualize = True\n")


def child(script, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("PXA_OPERAND_DTYPE", "PXA_LIB_PATH")}
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_scripts", script), *[str(a) for a in args]],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    print("\n" + r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_train_py_ema_checkpoint_pictures_and_load_ema(tmp_path):
    cfg, feats, w = tmp_path / "cfg.py", tmp_path / "feats", tmp_path / "w"
    cfg.write_text(CFG + "optimizer = dict(type='AdamW', lr=1e-2, weight_decay=3e-2, eps=1e-10)\n")
    write_feats(feats, 2)
    out = child("train.py", cfg, "--synthetic", "--max-steps", "2", "--ema", "--visualize", "--validation-feats", feats, "--work-dir", w)
    assert "EMA of the weights at rate 0.5" in out
    ck = torch.load(w / "checkpoints" / "epoch_1_step_2.pth", map_location="cpu", weights_only=False)
    sd, se = ck["state_dict"], ck["state_dict_ema"]
    assert list(sd) == list(se) and all(sd[k].shape == se[k].shape for k in sd)
    assert all(torch.isfinite(v).all() for v in se.values()) and any(not torch.equal(sd[k], se[k]) for k in sd)
    for d in ("step_1", "step_1_ema"):
        assert sorted(os.listdir(w / "validation" / d)) == ["0.png", "1.png"]
    assert sorted(os.listdir(w / "validation")) == ["step_1", "step_1_ema"]                    # step 2 is no multiple of eval_sampling_steps
    # resume from the averaged weights: with lr = 0 the step leaves them as they were loaded
    cfg.write_text(CFG.replace("save_model_steps = 2", "save_model_steps = 1") + "optimizer = dict(type='AdamW', lr=0.0, weight_decay=3e-2, eps=1e-10)\n")
    out = child("train.py", cfg, "--synthetic", "--max-steps", "1", "--ema", "--load-ema", "--resume-from", w / "checkpoints" / "epoch_1_step_2.pth", "--work-dir", w)
    ck3 = torch.load(w / "checkpoints" / "epoch_1_step_3.pth", map_location="cpu", weights_only=False)
    assert all(torch.equal(ck3["state_dict"][k], se[k]) and torch.equal(ck3["state_dict_ema"][k], se[k]) for k in se)


def test_train_lora_py_writes_the_averaged_adapters(tmp_path):
    from safetensors.torch import load_file
    cfg, feats, w = tmp_path / "cfg.py", tmp_path / "feats", tmp_path / "w"
    cfg.write_text(CFG)
    write_feats(feats, 2)
    child("train_lora.py", cfg, "--synthetic", "--max-steps", "2", "--rank", "4", "--lr", "1e-2", "--ema", "--visualize", "--validation-feats", feats, "--work-dir", w)
    for d in ("step_1", "step_1_ema"):
        assert sorted(os.listdir(w / "validation" / d)) == ["0.png", "1.png"]
    for raw, avg in ((w / "lora", w / "lora_ema"), (w / "checkpoints" / "lora_step_2", w / "checkpoints" / "lora_ema_step_2")):
        assert json.loads((avg / "adapter_config.json").read_text()) == json.loads((raw / "adapter_config.json").read_text())
        a, b = load_file(str(raw / "adapter_model.safetensors")), load_file(str(avg / "adapter_model.safetensors"))
        assert list(a) == list(b) and all(a[k].shape == b[k].shape and torch.isfinite(b[k]).all() for k in a)
    # the loader scripts/inference.py --lora_path uses takes the averaged directory (shapes and names are checked there; no weights are needed for that)
    from pixart_sigma_amd import PixArtMS_XL_2
    with torch.device("meta"):
        m = PixArtMS_XL_2(input_size=32, model_max_length=16)
    lo = m.load_lora(str(w / "lora_ema"))
    assert lo.config.r == 4 and len(lo.params) == len(b)
