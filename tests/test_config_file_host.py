"""train_scripts/config_file.py: the config reader with `_base_` inheritance and the operand-type choice the training scripts make before they import
the library.  No GPU, no torch."""
import importlib.util
import os
import subprocess
import sys

import pytest

from conftest import ROOT

PATH = os.path.join(ROOT, "train_scripts", "config_file.py")


@pytest.fixture(scope="module")
def cf():
    spec = importlib.util.spec_from_file_location("config_file_host", PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_base_inheritance_over_two_levels(cf, tmp_path):
    (tmp_path / "sub").mkdir()
    (tmp_path / "root.py").write_text("import os\na = 1\nb = 1\nc = 1\n_hidden = 1\ndef f():\n    pass\n")
    (tmp_path / "sub" / "mid.py").write_text("_base_ = ['../root.py']\nb = 2\nc = 2\n")
    (tmp_path / "sub" / "leaf.py").write_text("_base_ = 'mid.py'\nc = 3\n")                             # relative to the file; a string or a list
    assert cf.run_config(str(tmp_path / "sub" / "leaf.py")) == {"a": 1, "b": 2, "c": 3}


def test_circular_base_exits(cf, tmp_path):
    (tmp_path / "x.py").write_text("_base_ = ['y.py']\n")
    (tmp_path / "y.py").write_text("_base_ = ['x.py']\n")
    with pytest.raises(SystemExit, match="circular _base_"):
        cf.run_config(str(tmp_path / "x.py"))


def early(cf, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["train.py", *argv])
    monkeypatch.setenv("PXA_OPERAND_DTYPE", "unset below")             # so that monkeypatch records the variable's state before the test
    monkeypatch.delenv("PXA_OPERAND_DTYPE")
    return cf.early_mixed_precision(sys.argv[1:]), os.environ.get("PXA_OPERAND_DTYPE")


def test_early_mixed_precision(cf, monkeypatch, tmp_path):
    bf16, fp16, no = (tmp_path / n for n in ("bf16.py", "fp16.py", "no.py"))
    bf16.write_text("mixed_precision = 'bf16'\n")
    fp16.write_text("mixed_precision = 'fp16'\n")
    no.write_text("mixed_precision = 'no'\n")
    assert early(cf, monkeypatch, str(bf16), "--mixed-precision", "fp16", "--synthetic") == ("fp16", "f16")      # the command line wins
    assert early(cf, monkeypatch, "--mixed-precision=fp16", str(bf16)) == ("fp16", "f16")
    assert early(cf, monkeypatch, str(fp16), "--max-steps", "2") == ("fp16", "f16")
    assert early(cf, monkeypatch, str(fp16), "--mixed-precision", "bf16") == ("bf16", None)
    assert early(cf, monkeypatch, str(bf16)) == ("bf16", None)
    assert early(cf, monkeypatch, "--synthetic") == ("bf16", None)                                               # no config, no flag
    with pytest.raises(SystemExit, match=r"mixed_precision='no': this path computes with bf16 or fp16 MFMA operands only"):
        early(cf, monkeypatch, str(no))
    assert "PXA_OPERAND_DTYPE" not in os.environ


def test_the_config_is_executed_even_when_the_command_line_decides(cf, monkeypatch, tmp_path):
    (tmp_path / "loop.py").write_text("_base_ = ['loop.py']\n")
    with pytest.raises(SystemExit, match="circular _base_"):
        early(cf, monkeypatch, str(tmp_path / "loop.py"), "--mixed-precision", "fp16")
    assert "PXA_OPERAND_DTYPE" not in os.environ


def test_imports_without_torch_or_the_library():
    code = (f"import importlib.util, sys\nspec = importlib.util.spec_from_file_location('config_file', {PATH!r})\n"
            "mod = importlib.util.module_from_spec(spec)\nspec.loader.exec_module(mod)\n"
            "assert callable(mod.run_config) and callable(mod.early_mixed_precision)\n"
            "assert 'torch' not in sys.modules and 'pixart_sigma_amd' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
