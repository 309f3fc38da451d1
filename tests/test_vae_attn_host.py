"""Host side of the streaming VAE mid-block attention (pxa_vae_attn, ABI 11): which path AutoencoderKL takes (vae.autoencoder_kl.attention_plan, a pure
function), how the mode is chosen (set_attention over PXA_VAE_ATTN over "auto"), and the new entry at the drop-in boundary.  No GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _plan():
    from pixart_sigma_amd.vae.autoencoder_kl import attention_plan
    return attention_plan


@pytest.mark.parametrize("HW", [8, 4096, 65536])
def test_auto_keeps_the_scores_path_up_to_the_2k_config(HW):
    assert _plan()("auto", HW, 512) == "scores"
    assert _plan()("auto", HW, 256) == "scores"


def test_auto_streams_above_65536_tokens():
    assert _plan()("auto", 65537, 512) == "streaming"
    assert _plan()("auto", 4 * 65536, 256) == "streaming"


@pytest.mark.parametrize("HW", [1, 7, 8, 4096, 65536, 65537])
def test_explicit_modes_are_honoured(HW):
    for C in (512, 256):
        assert _plan()("scores", HW, C) == "scores"
        assert _plan()("streaming", HW, C) == "streaming"


def test_streaming_with_an_unbuilt_width_raises_and_auto_does_not():
    with pytest.raises(ValueError):
        _plan()("streaming", 4096, 384)
    for HW in (8, 4096, 65536, 65537):                    # "auto" never fails where "scores" would have run
        assert _plan()("auto", HW, 384) == "scores"
    assert _plan()("scores", 4096, 384) == "scores"


def test_unknown_mode_raises():
    from pixart_sigma_amd.vae import AutoencoderKL
    with pytest.raises(ValueError):
        _plan()("flash", 4096, 512)
    vae = AutoencoderKL(block_out_channels=(128,), layers_per_block=1)
    with pytest.raises(ValueError):
        vae.set_attention("flash")
    assert vae.attention_mode() in ("auto", os.environ.get("PXA_VAE_ATTN"))      # the failed call changed nothing


def test_set_attention_beats_the_environment(monkeypatch):
    from pixart_sigma_amd.vae import AutoencoderKL
    vae = AutoencoderKL(block_out_channels=(128,), layers_per_block=1)
    monkeypatch.delenv("PXA_VAE_ATTN", raising=False)
    assert vae.attention_mode() == "auto"
    monkeypatch.setenv("PXA_VAE_ATTN", "streaming")       # read per call, like the other PXA_VAE_* switches
    assert vae.attention_mode() == "streaming"
    monkeypatch.setenv("PXA_VAE_ATTN", "scores")
    assert vae.attention_mode() == "scores"
    assert vae.set_attention("streaming") is vae
    assert vae.attention_mode() == "streaming"
    vae.set_attention("auto")
    assert vae.attention_mode() == "auto"
    monkeypatch.setenv("PXA_VAE_ATTN", "flash")           # an unknown value from the environment is an error where the plan is made
    fresh = AutoencoderKL(block_out_channels=(128,), layers_per_block=1)
    with pytest.raises(ValueError):
        _plan()(fresh.attention_mode(), 64, 512)


def test_entry_is_declared_exported_and_bound():
    from pixart_sigma_amd import build, lib
    src = open(os.path.join(ROOT, "include", "pixart_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+pxa_vae_attn\s*\(([^)]*)\)\s*;", code)
    assert m, "pxa_vae_attn is not declared in include/pixart_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 13 == len(lib.SIGNATURES["pxa_vae_attn"])
    kinds = [lib.c_void_p if "*" in p or "hipStream_t" in p else lib.c_long if p.startswith("long") else lib.c_float if p.startswith("float") else lib.c_int
             for p in params]
    assert kinds == lib.SIGNATURES["pxa_vae_attn"]
    assert re.search(r"#define\s+PXA_ABI_VERSION\s+11\b", src)
    dll = ctypes.CDLL(build.build())
    assert hasattr(dll, "pxa_vae_attn")
    assert dll.pxa_abi_version() == 11


def test_binding_abi_version():
    from pixart_sigma_amd import lib
    assert lib.ABI_VERSION == 11
