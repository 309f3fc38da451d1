"""Loader of the T5 fixtures tools/make_t5_golden.py writes: tests/golden/t5_<name>.pt plus its part files (the state dict and the hidden states, cut below
the repository's file-size limit), put together as one dict.  Loaded once per process and handed out unchanged: callers must not write into the tensors."""
import functools
import json
import os

import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load(name):
    fx = torch.load(os.path.join(GOLDEN_DIR, name + ".pt"), weights_only=False)
    sd, hs = {}, {}
    for part in fx["parts"]:
        for k, v in torch.load(os.path.join(GOLDEN_DIR, part), weights_only=False).items():
            kind, _, key = k.partition(".")
            if kind == "state_dict":
                sd[key] = v
            else:
                hs[int(key)] = v
    fx["state_dict"] = sd
    fx["hidden_states"] = [hs[i] for i in range(len(hs))]
    return fx


@functools.lru_cache(maxsize=None)
def ref_noise():
    with open(os.path.join(GOLDEN_DIR, "t5_ref_noise.json")) as f:
        return json.load(f)
