"""LoRA adapters on a depth-2 PixArtMS (weights and inputs from oracle.weights, as tests/test_model_gpu.py builds them; ragged text lengths; one case with KV
compression 'conv' on block 1, one with qk_norm) against a PLAIN model that carries the host-merged fp32 weights W + s B A.  That plain path - forward, loss and
every weight gradient - is pinned to the reference by the train goldens, so the adapter gradients are checked against its dW projected on the host in fp64
(dA = s B^T dW, dB = s dW A^T per row slice).  Runs under either operand build (tests/test_lora_f16_gpu.py re-runs the file under f16); the tolerances are those
of tests/test_model_gpu.py:26-35."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from oracle import pixart_oracle as po  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402
from pixart_sigma_amd import lib as _lib  # noqa: E402
from pixart_sigma_amd.lora import BLOCK_MODULES, LoraConfig  # noqa: E402

F16 = _lib.OPERAND == "f16"
FWD_RP_TOL = 1e-3 if F16 else 3e-3
LOSS_TOL = 1e-3 if F16 else 5e-3
GRAD_TOL = 1.2e-3 if F16 else 3e-2
GRAD_TOL_DEEP = 1.5e-3 if F16 else 3e-2          # (depth 28; no test of this file is that deep)
CASES = ["train_d2", "train_d2_qknorm"]          # KV compression 'conv' x2 on block 1; qk_norm.  Both: B = 2, lens [20, 9]
RANK = 4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _plain(g, sd, train=False):
    from pixart_sigma_amd import build_model
    cfg = po.OracleCfg(**g["cfg"])
    kvc = None
    if cfg.kv_sampling is not None:
        kvc = {"sampling": cfg.kv_sampling, "scale_factor": cfg.kv_scale_factor, "kv_compress_layer": list(cfg.kv_layers)}
    m = build_model("PixArtMS", depth=cfg.depth, hidden_size=1152, num_heads=16, input_size=cfg.input_size, pe_interpolation=cfg.pe_interpolation,
                    model_max_length=cfg.model_max_length, class_dropout_prob=0.0, kv_compress_config=kvc, qk_norm=cfg.qk_norm, micro_condition=cfg.micro_condition)
    m.load_state_dict(sd)
    m = m.cuda()
    m.train(train)
    return m


_SHARED = {}


def _setup(golden, name):
    """Per case, made once and left unchanged: base weights, inputs, random adapters scaled to ||s B A|| = 0.25 ... 0.5 ||W|| per module, the host-merged
    state dict."""
    if name not in _SHARED:
        g = golden(name)
        cfg = po.OracleCfg(**g["cfg"])
        sd = make_state_dict(cfg, seed=g["weights_seed"])
        inp = make_inputs(seed=g["inputs_seed"], **g["inputs"])
        config = LoraConfig(r=RANK, target_modules=list(BLOCK_MODULES))
        s = config.scaling
        gen = torch.Generator().manual_seed(11)
        ad, merged = {}, {k: v.clone() for k, v in sd.items()}
        for i in range(cfg.depth):
            for j, (mod, (lin, sl, n)) in enumerate(BLOCK_MODULES.items()):
                w = sd[f"blocks.{i}.{lin}.weight"]
                rows = w.shape[0] // n
                lo, hi = sl * rows, (sl + 1) * rows
                a, bt = torch.randn(RANK, w.shape[1], generator=gen), torch.randn(RANK, rows, generator=gen)
                delta = bt.double().t() @ a.double()
                frac = 0.25 + 0.25 * ((i * 10 + j) % 5) / 4
                wn = w[lo:hi].double().norm().item()
                bt = (bt * (frac * (wn if wn > 0 else 1.0) / (s * delta.norm().item()))).float()
                ad[f"blocks.{i}.{mod}"] = (a, bt, lin, lo, hi)
                merged[f"blocks.{i}.{lin}.weight"][lo:hi] = (w[lo:hi].double() + s * (bt.double().t() @ a.double())).float()
        _SHARED[name] = dict(g=g, cfg=cfg, sd=sd, inp=inp, config=config, ad=ad, merged=merged)
    return _SHARED[name]


def _with_adapters(c, train=False, random=True):
    m = _plain(c["g"], c["sd"], train)
    lo = m.add_lora(c["config"])
    if random:
        with torch.no_grad():
            for n, (a, bt, *_rest) in c["ad"].items():
                lo.params[n + ".lora_A"].copy_(a)
                lo.params[n + ".lora_Bt"].copy_(bt)
    return m


def _args(c):
    inp = c["inp"]
    return inp["x"].cuda(), inp["t"].cuda(), inp["y"].cuda(), inp["mask"].cuda()


def _fwd(m, c):
    x, t, y, mask = _args(c)
    with torch.no_grad():
        return m(x, t, y, mask=mask)


def _backward_scaled(make_loss, grad):
    """tests/test_model_gpu.py's protocol on the flat gradient buffer `grad`: fp16 operands - the loss is scaled by the largest power of two <= 2^16 whose
    gradients stay finite, and the buffer is unscaled afterwards."""
    scale = 65536.0 if F16 else 1.0
    while True:
        grad.zero_()
        terms = make_loss()
        (terms["loss"].mean() * scale).backward()
        if not F16 or torch.isfinite(grad).all() or scale <= 1.0:
            break
        scale /= 2
    if scale != 1.0:
        grad.div_(scale)
    return terms, scale


def _loss_fn(m, c):
    from pixart_sigma_amd import IDDPM
    diff = IDDPM(str(1000), learn_sigma=True, pred_sigma=True, snr=False)
    x, _, y, mask = _args(c)
    kw = dict(y=y, mask=mask[:, None, None, :], data_info=c["g"].get("data_info"))
    return lambda: diff.training_losses(m, x, c["g"]["t"].cuda(), model_kwargs=kw, noise=c["inp"]["noise"].cuda())


# ---------------------------------------------------------------------------------------------- 1. fresh adapters
@pytest.mark.parametrize("name", CASES)
def test_fresh_adapters_leave_the_forward_bit_equal(golden, name):
    c = _setup(golden, name)
    m = _plain(c["g"], c["sd"])
    y0 = _fwd(m, c)
    shadow0 = m._store.shadow.clone()
    m.add_lora(c["config"])                                 # gaussian init: B = 0
    y1 = _fwd(m, c)
    assert m._engine.lora is m._lora and len(m.lora_parameters()) == 2 * 10 * 2
    assert torch.equal(m._store.shadow.view(torch.int16), shadow0.view(torch.int16))
    assert torch.equal(y1, y0)


# ---------------------------------------------------------------------------------------------- 2. random adapters vs the plain merged model
@pytest.mark.parametrize("name", CASES)
def test_random_adapters_match_the_plain_merged_model(golden, name):
    c = _setup(golden, name)
    m, ref = _with_adapters(c), _plain(c["g"], c["merged"])
    y, y_ref, y_base = _fwd(m, c), _fwd(ref, c), _fwd(_plain(c["g"], c["sd"]), c)
    e = rel_l2(y, y_ref)
    away = rel_l2(y_base, y_ref)
    print(f"\n[{name}] forward with adapters vs plain merged model rel-L2 {e:.2e} (bound {FWD_RP_TOL:.0e}); the base model is {away:.2e} away")
    record_parity(f"lora {name}: forward vs plain merged model", e, FWD_RP_TOL)
    assert torch.isfinite(y).all() and away > 0.05            # the adapters matter: a missing slice or scale is far above the tolerance
    assert e <= FWD_RP_TOL
    m.train(), ref.train()
    with torch.no_grad():
        l, l_ref = _loss_fn(m, c)()["loss"], _loss_fn(ref, c)()["loss"]
    e = rel_l2(l.cpu(), l_ref.cpu())
    print(f"[{name}] training_losses {l.tolist()} vs {l_ref.tolist()}: rel {e:.2e} (bound {LOSS_TOL:.0e})")
    record_parity(f"lora {name}: loss vs plain merged model", e, LOSS_TOL)
    assert e <= LOSS_TOL


# ---------------------------------------------------------------------------------------------- 3. gradients
@pytest.mark.parametrize("name", CASES)
def test_adapter_gradients_match_the_projected_weight_gradients(golden, name):
    from pixart_sigma_amd.model.utils import set_grad_checkpoint
    c = _setup(golden, name)
    s = c["config"].scaling
    ref = _plain(c["g"], c["merged"], train=True)
    ref._prepare(torch.device("cuda"))
    _backward_scaled(_loss_fn(ref, c), ref._store.grad)
    dW = {k: p.grad.detach().double().cpu() for k, p in ref.named_parameters() if k.endswith(".weight") and k.startswith("blocks.")}
    del ref
    m = _with_adapters(c, train=True)
    m._prepare(torch.device("cuda"))
    A = m._lora.store
    m._store.grad.fill_(1.25)                                # the base gradient buffer: nothing may land in it
    master0 = m._store.master.clone()
    _, scale = _backward_scaled(_loss_fn(m, c), A.grad)
    assert bool((m._store.grad == 1.25).all()) and torch.equal(m._store.master, master0)
    worst = (0.0, None)
    for n, (a, bt, lin, lo, hi) in c["ad"].items():
        i = n.split(".")[1]
        dw = dW[f"blocks.{i}.{lin}.weight"][lo:hi]
        for leaf, want in (("lora_A", s * bt.double() @ dw), ("lora_Bt", s * a.double() @ dw.t())):
            e = rel_l2(A.g(f"{n}.{leaf}").cpu(), want)
            worst = max(worst, (e, f"{n}.{leaf}"))
            assert e <= GRAD_TOL, (n, leaf, e)
    print(f"\n[{name}] worst adapter gradient vs projected dW of the plain merged model: {worst[0]:.2e} ({worst[1]}; bound {GRAD_TOL:.1e}); loss scale {scale:g}")
    record_parity(f"lora {name}: worst adapter gradient ({worst[1]})", worst[0], GRAD_TOL)
    for p in m.lora_parameters():                             # gradients live in the adapters' flat buffer
        assert p.grad is not None and p.grad.untyped_storage().data_ptr() == A.grad.untyped_storage().data_ptr()
    # grad_checkpointing=True recomputes every block from its input and goes through the same block_bwd: the same bits
    saved = A.grad.clone()
    set_grad_checkpoint(m)
    A.grad.zero_()
    (_loss_fn(m, c)()["loss"].mean() * scale).backward()
    if scale != 1.0:
        A.grad.div_(scale)                                    # the same unscaling the saved run got
    assert bool((m._store.grad == 1.25).all())
    e = rel_l2(A.grad, saved)
    record_parity(f"lora {name}: checkpointed vs saved-activation adapter gradients (bit-equal asked)", e, 0.0)
    assert torch.equal(A.grad, saved), f"checkpointed and saved-activation adapter gradients differ: rel-L2 {e:.2e}"


# ---------------------------------------------------------------------------------------------- 4. optimizer, caches, graphs
@pytest.mark.parametrize("name", CASES[:1])
def test_two_adamw_steps_update_adapters_only_and_nothing_goes_stale(golden, name, monkeypatch):
    from pixart_sigma_amd import DPMS, ops
    from pixart_sigma_amd.dp import FusedAdamW, LossScaler
    c = _setup(golden, name)
    m = _with_adapters(c, train=True)
    m._prepare(torch.device("cuda"))
    S, A = m._store, m._lora.store
    scaler = LossScaler("cuda", init_scale=256.0) if F16 else None
    opt = FusedAdamW(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, scaler=scaler)
    assert opt.store is A and opt.m.numel() == A.total
    master0, adapters0 = S.master.clone(), A.master.clone()
    y_before = _fwd(m, c)                                     # an inference forward: fills Engine._text_cache
    assert m._engine._text_cache is not None
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = _loss_fn(m, c)()["loss"].mean()
        losses.append(loss.item())
        (scaler.scale(loss) if scaler else loss).backward()
        opt.step()
    with torch.no_grad():
        losses.append(_loss_fn(m, c)()["loss"].mean().item())
    print(f"\n[{name}] loss over two adapter steps: {losses}")
    assert torch.equal(S.master, master0) and not torch.equal(A.master, adapters0)           # the base master: bit-unchanged
    assert losses[2] != losses[0] and all(l == l for l in losses)
    if scaler is not None:
        assert scaler.steps_applied == 2
    # shadow (and the prescaled qkv copy) = a fresh merge of the updated adapters
    D = 1152
    for lname, slices in m._lora.slices.items():
        fresh = ops.cast_bf16(S.f(lname + ".weight"))
        qs = None
        if m._engine._qs is not None and lname.endswith("attn.qkv"):
            l = int(lname.split(".")[1])
            qs = torch.empty_like(m._engine._qs[0][l])
            ops.scale_copy(S.f(lname + ".weight").view(-1), 0, 1, D * D, 3 * D * D, ops.Q_PRESCALE, out_bf16=qs.view(1, -1))
        for lo, hi, ad in slices:
            ops.lora_merge(S.f(lname + ".weight"), lo, hi, A.f(ad + ".lora_A"), A.f(ad + ".lora_Bt"), m._lora.scale, fresh, dst2=qs, mul_rows=(0, D), mul=ops.Q_PRESCALE)
        assert torch.equal(fresh.view(torch.int16), S.w(lname + ".weight").view(torch.int16)), lname
        if qs is not None:
            assert torch.equal(qs.view(torch.int16), m._engine._qs[0][l].view(torch.int16)), lname
    # the cached text branch is not stale: the same bits as with the cache off, and not what it gave before the steps
    m.eval()
    y_after = _fwd(m, c)
    monkeypatch.setenv("PXA_TEXT_CACHE", "0")
    y_nocache = _fwd(m, c)
    monkeypatch.delenv("PXA_TEXT_CACHE")
    assert torch.equal(y_after, y_nocache) and not torch.equal(y_after, y_before)
    # a captured sampling graph follows an adapter update (as test_graphed_sampler_follows_weight_updates does for a weight load)
    x, _, y, mask = _args(c)
    gen = torch.Generator().manual_seed(7)
    null_y = torch.randn(1, 1, y.shape[-2], 4096, generator=gen).repeat(x.shape[0], 1, 1, 1).cuda()
    solver = DPMS(m.forward_with_dpmsolver, condition=y, uncondition=null_y, cfg_scale=4.5, model_kwargs=dict(data_info=None, mask=c["inp"]["mask"]))
    kw = dict(steps=3, order=2, skip_type="time_uniform", method="multistep")
    g1 = solver.sample_graphed(x, **kw)
    assert torch.equal(g1, solver.sample(x, **kw))
    graph = solver._graph
    opt.zero_grad()
    loss = _loss_fn(m, c)()["loss"].mean()
    (scaler.scale(loss) if scaler else loss).backward()
    opt.step()
    g2 = solver.sample_graphed(x, **kw)
    assert solver._graph is graph
    assert torch.equal(g2, solver.sample(x, **kw)) and not torch.equal(g2, g1)


# ---------------------------------------------------------------------------------------------- 5. save / load / merge / scale
@pytest.mark.parametrize("name", CASES[1:])
def test_save_load_merge_and_scale(golden, name, tmp_path):
    c = _setup(golden, name)
    m = _with_adapters(c)
    y = _fwd(m, c)
    m.save_lora(str(tmp_path))
    m2 = _plain(c["g"], c["sd"])
    y_base = _fwd(m2, c)
    m2.load_lora(str(tmp_path))
    assert torch.equal(_fwd(m2, c), y)                        # save -> new model -> load: the same bits
    m2.set_lora_scale(0.0)
    assert torch.equal(_fwd(m2, c), y_base)                   # scale 0: the base model's bits
    m2.set_lora_scale(1.0)
    assert torch.equal(_fwd(m2, c), y)
    m2.merge_and_unload()
    assert m2._lora is None and m2._engine.lora is None and m2.lora_parameters() == [] and not any("lora" in k for k in m2.state_dict())
    y_m = _fwd(m2, c)
    e = rel_l2(y_m, y)
    print(f"\n[{name}] forward after merge_and_unload vs with adapters: rel-L2 {e:.2e} (bound {FWD_RP_TOL:.0e})")
    record_parity(f"lora {name}: merge_and_unload forward vs adapted forward", e, FWD_RP_TOL)
    assert e <= FWD_RP_TOL
    w = m2.state_dict()["blocks.1.mlp.fc1.weight"].cpu()
    assert rel_l2(w, c["merged"]["blocks.1.mlp.fc1.weight"]) < 1e-6          # the fp32 master now carries W + s B A
    m2._store.refresh_shadow(force=True)                      # a re-cast of the merged master rounds to what the merge had put in the shadow
    assert torch.equal(_fwd(m2, c), y_m)
