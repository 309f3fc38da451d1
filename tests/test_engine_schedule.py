"""The launch schedule of engine.Engine, pinned: per case of tests/ops_trace.py, the calls the engine makes on the CPU stand-ins - every op, every argument
by name, every buffer by identity, offset, shape and strides, every grad_ready_hook firing - equal tests/golden/engine_schedule_<case>.txt line for line.
The fixtures were recorded before engine.py was restructured (their first line names the commit) and are not regenerated with it: a refactor of the
sequencing passes when the kernels still receive the same launches, in the same order, on the same buffers."""
import pytest

import ops_trace


@pytest.mark.parametrize("case", list(ops_trace.CASES))
def test_schedule_equals_the_recorded_one(case):
    with open(ops_trace.fixture(case)) as f:
        want = f.read().splitlines()[1:]                  # the first line names the commit of the recording
    got = ops_trace.CASES[case]()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            ctx = "\n".join(f"  {j + 2:4d}  {want[j]}" for j in range(max(0, i - 2), i))
            pytest.fail(f"{case}: first difference at line {i + 2} of the fixture\n{ctx}\n  want  {w}\n  got   {g}\n"
                        + "\n".join(f"  {j + 2:4d}  {want[j]}" for j in range(i + 1, min(len(want), i + 3))), pytrace=False)
    assert len(got) == len(want), f"{case}: {len(got)} lines traced, {len(want)} recorded; first extra line: {max(got, want, key=len)[min(len(got), len(want)):][:1]}"
