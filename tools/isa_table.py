"""One line per gfx950 kernel of the given sources: name, hash of its normalised instruction stream, the values of its kernel descriptor (the ones that matter most in
words, all of them as `desc=<hash>`).
    python tools/isa_table.py [--f16] csrc-file.hip [more.hip ...]  > table.txt
Each source is compiled to assembly with the library's flags (pixart_sigma_amd/build.py, per-file flags included; hipcc cross-compiles, no GPU needed).
A kernel's body runs from its label to its .Lfunc_end; comments go, and the function number inside local labels (.LBB<fn>_<n>) goes, so that a kernel that
moved to another file or another place in its file hashes the same.  Lines are sorted by kernel name (the source file is not printed): a refactor that
moves kernels between files without touching their code leaves `diff` of the two tables empty.  A name that appears twice is printed twice."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixart_sigma_amd import build as B

SHOWN = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("acc", "accum_offset"), ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"))


def kernels(text):
    """[(name, body hash, {descriptor key: value})] of one assembly file"""
    out = []
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        name = m.group(1)
        desc = dict(re.findall(r"^\s*\.amdhsa_(\S+) (\S+)", m.group(2), re.M))
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".Lfunc_end", start)]
        lines = []
        for l in body.split("\n"):
            l = re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", l.split(";")[0]).strip()
            if l:
                lines.append(l)
        out.append((name, hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], desc))
    return out


def table(srcs, extra):
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for src in srcs:
            src = os.path.abspath(src)
            o = os.path.join(td, os.path.basename(src) + ".s")
            subprocess.run([B._hipcc(), *B.FLAGS, *B.PER_FILE_FLAGS.get(os.path.basename(src), []), *extra, "-I", B.INCLUDE, "-I", B.CSRC,
                            "-S", "--cuda-device-only", src, "-o", o], check=True)
            rows += kernels(open(o).read())
    for name, h, desc in sorted(rows, key=lambda r: r[0]):
        rest = hashlib.sha256(repr(sorted(desc.items())).encode()).hexdigest()[:8]
        print(name, h, " ".join(f"{k}={desc.get(d, '-')}" for k, d in SHOWN), f"desc={rest}")


if __name__ == "__main__":
    args = sys.argv[1:]
    f16 = "--f16" in args
    table([a for a in args if a != "--f16"], ["-DPXA_OPERAND_F16"] if f16 else [])
