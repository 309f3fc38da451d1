"""Host side of the EMA / validation wiring: train_loop's call order with the two keyword arguments, the argument and config precedence, the start-up
exits, and WeightEMA's state dict on a CPU store.  No GPU; the fakes are in tests/ema_fakes.py."""
import importlib.util
import os
import types

import pytest
import torch

import ema_fakes as F
from conftest import ROOT


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def train():
    return _load("ema_host_train", "train_scripts", "train.py")


def cfg_of(train, **kw):
    return dict(train.DEFAULTS, log_interval=1000, **kw)


def args(**kw):
    return types.SimpleNamespace(**{**dict(ema=False, ema_rate=None, visualize=False, validation_feats=None, load_ema=False), **kw})


# ---------------------------------------------------------------------------------------------- train_loop
def test_without_the_flags_the_trace_is_todays(train):
    cfg = cfg_of(train, gradient_accumulation_steps=2, save_model_steps=2, eval_sampling_steps=1)
    old = F.run(train, cfg, 3, keywords=False)
    assert F.run(train, cfg, 3) == old
    assert "ema.update" not in old and not any(isinstance(e, tuple) and e[0] == "validate" for e in old)
    step = ["zero_grad", ("lr", 1.0), "next", "training_losses", "no_sync enter", "backward", "no_sync exit", "next", "training_losses", "backward", "opt.step", "sched.step"]
    assert old == step + step + [("save", 2)] + step


def test_ema_update_sits_directly_behind_opt_step_once_per_optimizer_step(train):
    cfg = cfg_of(train, gradient_accumulation_steps=3, save_model_steps=2, eval_sampling_steps=1)
    plain = F.run(train, cfg, 4)
    with_ema = F.run(train, cfg, 4, ema=True)
    want = []
    for e in plain:
        want += [e, "ema.update"] if e == "opt.step" else [e]
    assert with_ema == want and with_ema.count("ema.update") == 4 == with_ema.count("opt.step")
    assert with_ema.count("training_losses") == 12


def test_validation_runs_after_step_1_and_every_kth_step_on_rank_0(train, capsys):
    cfg = cfg_of(train, save_model_steps=4, eval_sampling_steps=3)
    tr = F.run(train, cfg, 7, ema=True, validate=True)
    assert [e[1] for e in tr if isinstance(e, tuple) and e[0] == "validate"] == [1, 3, 6]
    plain = F.run(train, cfg, 7, ema=True)
    assert [e for e in tr if not (isinstance(e, tuple) and e[0] == "validate")] == plain
    i = tr.index(("validate", 3))
    assert tr[i - 3:i] == ["opt.step", "ema.update", "sched.step"]                    # behind the whole step
    tr = F.run(train, dict(cfg, log_interval=1), 4, validate=True)
    assert tr[tr.index(("validate", 3)) + 1] == "zero_grad" and tr.index(("validate", 3)) < tr.index(("save", 4))
    assert capsys.readouterr().out.count("\n") == 4                                    # the log lines; validation comes behind each
    # a resumed run counts the job's steps: 5 + 1 = 6 is due, 7 is not; step 1 of the job is long past
    tr = F.run(train, cfg, 2, start_step=5, validate=True)
    assert [e[1] for e in tr if isinstance(e, tuple) and e[0] == "validate"] == [6]
    assert not any(isinstance(e, tuple) and e[0] == "validate" for e in F.run(train, cfg, 7, rank=1, validate=True))


def test_validate_and_save_on_one_step_validation_first(train):
    cfg = cfg_of(train, save_model_steps=3, eval_sampling_steps=3)
    tr = F.run(train, cfg, 3, validate=True)
    assert tr[-2:] == [("validate", 3), ("save", 3)]


# ---------------------------------------------------------------------------------------------- arguments and config
def test_ema_rate_precedence(train, tmp_path):
    assert train.ema_decay(args(), cfg_of(train, ema_rate=0.99)) is None                # the config key alone means nothing
    assert train.ema_decay(args(ema=True), cfg_of(train)) == 0.9999
    assert train.ema_decay(args(ema=True), cfg_of(train, ema_rate=0.99)) == 0.99
    assert train.ema_decay(args(ema=True, ema_rate=0.5), cfg_of(train, ema_rate=0.99)) == 0.5
    assert train.ema_decay(args(ema=True, ema_rate=0.0), cfg_of(train, ema_rate=0.99)) == 0.0
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(SystemExit, match=r"must lie in \[0, 1\)"):
            train.ema_decay(args(ema=True, ema_rate=bad), cfg_of(train))
    with pytest.raises(SystemExit, match="--ema-rate needs --ema"):
        train.ema_decay(args(ema_rate=0.5), cfg_of(train))
    # the keys reach the config dict from a file, and none of them is refused
    p = tmp_path / "c.py"
    p.write_text("ema_rate = 0.95\nvisualize = True\neval_sampling_steps = 7\nvalidation_prompts = ['a', 'b']\n")
    cfg = train.load_config(str(p))
    assert (cfg["ema_rate"], cfg["eval_sampling_steps"], cfg["validation_prompts"]) == (0.95, 7, ["a", "b"])
    assert train.ema_decay(args(ema=True), cfg) == 0.95
    base = train.load_config(None)
    assert (base["ema_rate"], base["validation_prompts"], base["eval_sampling_steps"]) == (None, None, 250)


def test_visualize_needs_a_feature_source_at_start_up(train, tmp_path):
    cfg = cfg_of(train, validation_prompts=["dog", "cat"], eval_sampling_steps=5)
    assert train.check_visualize(args(), cfg, False) == []                              # off: nothing is checked, nothing is sampled
    with pytest.raises(SystemExit) as e:
        train.check_visualize(args(visualize=True), cfg, False)
    assert "--validation-feats" in str(e.value) and "text captions" in str(e.value) and "load_t5_feat = False" in str(e.value)
    assert train.check_visualize(args(visualize=True), cfg, True) == ["dog", "cat"]     # text captions: the T5 encoder makes them
    assert train.check_visualize(args(visualize=True, validation_feats=str(tmp_path)), cfg, False) == ["dog", "cat"]
    with pytest.raises(SystemExit, match="not a directory"):
        train.check_visualize(args(visualize=True, validation_feats=str(tmp_path / "none")), cfg, False)
    with pytest.raises(SystemExit, match="validation_prompts"):
        train.check_visualize(args(visualize=True, validation_feats=str(tmp_path)), cfg_of(train), False)
    with pytest.raises(SystemExit, match="eval_sampling_steps"):
        train.check_visualize(args(visualize=True, validation_feats=str(tmp_path)), dict(cfg, eval_sampling_steps=0), False)
    # a features directory that lacks a prompt's file is named with what it lacks
    from pixart_sigma_amd.validation import load_validation_feats
    with pytest.raises(SystemExit, match=r"missing \['0.npz', '1.npz', 'null.npz'\]"):
        load_validation_feats(str(tmp_path), 2, 8, "cpu")


def test_validation_feats_layout(tmp_path):
    import numpy as np
    from pixart_sigma_amd.validation import load_validation_feats
    for i, name in enumerate(["0", "1", "null"]):
        np.savez(tmp_path / f"{name}.npz", caption_feature=np.full((1, 12, 16), float(i), dtype=np.float32), attention_mask=np.array([[1] * (i + 1) + [0] * (11 - i)]))
    feats, masks, null = load_validation_feats(str(tmp_path), 2, 8, "cpu")
    assert tuple(feats.shape) == (2, 1, 8, 16) and tuple(masks.shape) == (2, 8) and tuple(null.shape) == (1, 1, 8, 16)
    assert feats[1].unique().tolist() == [1.0] and null.unique().tolist() == [2.0] and masks.sum(1).tolist() == [1, 2]


def test_missing_state_dict_ema_is_named_with_the_file(train, monkeypatch):
    sd = {"state_dict": {"w": torch.zeros(1)}}
    with pytest.raises(SystemExit, match=r"some/file\.pth: the checkpoint has no state_dict_ema"):
        train.ema_weights_of(sd, "some/file.pth")
    with pytest.raises(SystemExit, match="no state_dict_ema"):
        train.ema_weights_of({"w": torch.zeros(1)}, "bare.pth")
    both = {"state_dict": {"w": torch.zeros(1)}, "state_dict_ema": {"w": torch.ones(1)}}
    assert train.ema_weights_of(both, "f.pth") is both["state_dict_ema"]
    monkeypatch.setenv("PXA_OPERAND_DTYPE", os.environ.get("PXA_OPERAND_DTYPE", "bf16"))     # scripts/inference.py sets it at import: put back afterwards
    monkeypatch.setattr("sys.argv", ["inference.py"])
    inf = _load("ema_host_inference", "scripts", "inference.py")
    with pytest.raises(SystemExit, match=r"some/file\.pth: the checkpoint has no state_dict_ema"):
        inf.checkpoint_weights(sd, "some/file.pth", True)
    assert inf.checkpoint_weights(both, "f.pth", True) is both["state_dict_ema"] and inf.checkpoint_weights(both, "f.pth", False) is both["state_dict"]
    assert inf.checkpoint_weights(sd["state_dict"], "f.pth", False) is sd["state_dict"]


# ---------------------------------------------------------------------------------------------- WeightEMA on a CPU store
def test_weight_ema_state_dict_has_the_models_keys():
    from pixart_sigma_amd import PixArtMS
    from pixart_sigma_amd.ema import WeightEMA
    from pixart_sigma_amd.engine import ParamStore
    torch.manual_seed(0)
    m = PixArtMS(depth=1, input_size=8, model_max_length=8)
    with pytest.raises(AssertionError, match="prepare"):
        WeightEMA(m)
    m._store = ParamStore(m._ordered_named_params(), torch.device("cpu"), group_of=m._group_of)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        WeightEMA(m, decay=1.0)
    ema = WeightEMA(m, 0.9)
    assert ema.ema.numel() == m._store.total and torch.equal(ema.ema, m._store.master) and ema.ema.data_ptr() != m._store.master.data_ptr()
    sd, ref = ema.state_dict(), m.state_dict()
    assert list(sd) == list(ref)
    params = dict(m.named_parameters())
    for k, v in sd.items():
        assert v.shape == ref[k].shape and torch.equal(v, ref[k])
        inside = ema.ema.data_ptr() <= v.data_ptr() < ema.ema.data_ptr() + 4 * ema.ema.numel()
        assert inside == (k in params)                                   # parameters are views of the flat buffer, buffers are the model's own
    # load by name; buffers may come along, anything else is listed
    new = {k: v + 1 for k, v in sd.items()}
    ema.load_state_dict(new)
    assert all(torch.equal(ema.state_dict()[k], new[k]) for k in params)
    ema.load_state_dict({k: new[k] for k in params})                     # buffers are excepted
    first = next(iter(params))
    with pytest.raises(KeyError, match="missing.*" + first.replace(".", r"\.")):
        ema.load_state_dict({k: v for k, v in new.items() if k != first})
    with pytest.raises(KeyError, match="unexpected.*stray"):
        ema.load_state_dict(dict(new, stray=torch.zeros(1)))
    # a rebuilt store is noticed
    m._store = ParamStore(m._ordered_named_params(), torch.device("cpu"), group_of=m._group_of)
    with pytest.raises(RuntimeError, match="rebuilt its flat parameter store"):
        ema.update()
    with pytest.raises(RuntimeError, match="rebuilt its flat parameter store"):
        with ema.swapped():
            pass
