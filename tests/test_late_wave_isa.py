"""No GPU needed: the prologue of an X run as it is meant to be issued, pinned on the cross-compiled assembly of `slot_runx<2, 24, false, false>`
(kernels_slots.h slot_runx_lds_core, DESIGN.md 4.1b, profiles/late_wave/stamps.md).

The waves that are late at a run's first wave-slot ending are waves 4 .. 7, the second-dispatched wave of every SIMD, which lose the issue arbitration to
the older wave at equal priority.  The remedy that was kept: the younger half runs the prologue at priority 1, everybody the column loop at priority 0.
Its ordering property:

* ONE `s_setprio 1`, reached only through a SCALAR compare of the wave's first thread index against 256 and a scalar branch (s_setprio ignores EXEC: behind
  `s_and_saveexec` every wave would raise its priority, which is no priority at all);
* it stands before every vector load of the kernel -- before the entering cells are requested;
* ONE `s_setprio 0`, unconditional, behind the last load of the prologue and before the first column (`v_sad_u32`); no priority change inside the column loop
  (priority kept through the loop only swaps the two halves' roles) or behind it;
* the kernels whose workgroups share a CU carry no priority change at all: `slot_runx<2, 0, ...>` and `slot_groupx` stay as they were.
"""
import os
import re

import pytest

from test_isa_waits import HIPCC, _device_asm, _kernel


def _instructions(body):
    lines = [ln.strip() for ln in body.split("\n")]
    return [ln for ln in lines if ln and not ln.startswith(";") and not ln.startswith(".")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
def test_the_younger_half_of_an_x_run_has_priority_in_the_prologue_and_only_there():
    text = _device_asm()
    for frag in ("9slot_runxILi2ELi24ELb0ELb0E", "9slot_runxILi2ELi24ELb0ELb1E", "9slot_runxILi2ELi32ELb0ELb0E", "9slot_runxILi2ELi8ELb0ELb0E", "9slot_runxILi2ELi16ELb0ELb0E"):
        body, _ = _kernel(text, frag)
        ins = _instructions(body)
        prio = [(i, ln) for i, ln in enumerate(ins) if ln.startswith("s_setprio")]
        assert [ln.split()[1] for _, ln in prio] == ["1", "0"], (frag, prio)
        up, down = prio[0][0], prio[1][0]
        # the guard: a scalar compare against 256 and a scalar branch right in front, and no EXEC mask in play
        guard = ins[max(0, up - 4):up]
        assert any(re.match(r"s_cmpk?_(lt|ge|gt|le)_u32 s\d+, (0x100|256|0xff|255)$", ln) for ln in guard), (frag, guard)
        assert ins[up - 1].startswith("s_cbranch_scc"), (frag, guard)
        assert not any("saveexec" in ln for ln in ins[:up]), (frag, "the priority is raised under an EXEC mask: every wave would take it")
        # before the entering cells' request (and every other vector load); lowered behind the prologue's last load, before the first column
        loads = [i for i, ln in enumerate(ins) if ln.startswith("global_load")]
        sads = [i for i, ln in enumerate(ins) if re.match(r"v_sad_u32 v\d+, v\d+, s\d+, v\d+", ln)]
        assert loads and sads and up < loads[0], (frag, up, loads[:1])
        entering = [i for i, ln in enumerate(ins) if ln.startswith("global_load_dwordx4")]
        assert entering and all(up < i < down for i in entering), (frag, up, entering, down)
        assert max(i for i in loads if i < sads[0]) < down < sads[0], (frag, down, sads[0])
    for frag in ("9slot_runxILi2ELi0ELb0ELb0E", "9slot_runxILi2ELi0ELb0ELb1E", "11slot_groupxILi2ELb0E", "11slot_groupxILi3ELb0E"):
        body, _ = _kernel(text, frag)
        assert "s_setprio" not in body, frag
