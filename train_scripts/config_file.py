"""What the training scripts run before they import the library (standard library only: no torch, no pixart_sigma_amd): the config file reader and the
operand type, which is fixed when pixart_sigma_amd is imported."""
import argparse
import os
import runpy


def run_config(path, _seen=()):
    """A reference config file as a dict, with its `_base_` parents (mmcv convention, paths relative to the file: 13 of the reference configs inherit
    ../PixArt_xl2_internal.py) resolved first and overridden by the child."""
    path = os.path.abspath(path)
    if path in _seen:
        raise SystemExit(f"{path}: circular _base_")
    ns = runpy.run_path(path)
    out = {}
    bases = ns.get("_base_", [])
    for b in ([bases] if isinstance(bases, str) else bases):
        out.update(run_config(os.path.join(os.path.dirname(path), b), _seen + (path,)))
    out.update({k: v for k, v in ns.items() if not k.startswith("_") and not callable(v) and not isinstance(v, type(os))})
    return out


def early_mixed_precision(argv):
    """The MFMA operand type is a per-process choice (one library per type) and must be known before pixart_sigma_amd is imported:
    `mixed_precision = 'fp16'` in the config (every reference config: configs/PixArt_xl2_internal.py:57) selects the fp16-operand build +
    dynamic loss scaling, 'bf16' the bf16 build, 'no' / 'fp32' are refused (there is no fp32-operand MFMA path).  `--mixed-precision` on the command line
    (`argv`, without the program name) wins over the config, which is executed either way."""
    cfgs = [a for a in argv if a.endswith(".py") and os.path.exists(a)]
    mp = "bf16"
    if cfgs:
        mp = run_config(cfgs[0]).get("mixed_precision", "bf16")
    early = argparse.ArgumentParser(add_help=False)          # both `--mixed-precision fp16` and `--mixed-precision=fp16`
    early.add_argument("--mixed-precision", default=None)
    mp = early.parse_known_args(argv)[0].mixed_precision or mp
    if mp not in ("fp16", "bf16"):
        raise SystemExit(f"mixed_precision={mp!r}: this path computes with bf16 or fp16 MFMA operands only")
    if mp == "fp16":
        os.environ["PXA_OPERAND_DTYPE"] = "f16"
    return mp
