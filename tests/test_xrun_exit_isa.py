"""No GPU needed: the exit of an X run, pinned on the cross-compiled assembly of `slot_runx<2, XC, false, SPEC>` for XC = 8, 16, 24, 32
(kernels_slots.h slot_exit_cells and its parts, slot_runx_lds_core, DESIGN.md 4.1b "the exit", profiles/xrun_exit/).

A launch is a link of a chain of dependent launches, so what a kernel does behind its column loop is covered by no other wave.  The exit used to form
the thread's exit index there, bit by bit from the position table: 24 `v_bfe_u32`, 23 `v_lshl_or_b32` and the scalar shifts that unpack `out_pos`, about 110
instructions on the path of a headline run.  None of it depends on the cells.  What the kernels are meant to do instead:

* the gather stands in the PROLOGUE, behind its last vector request and in front of the first wait for a loaded word, where a wave sat idle;
* one VGPR (the exit index, or all ones for a thread that does not write) and one SGPR (the store form) travel through the loop;
* behind the last record store nothing gathers, nothing unpacks `out_pos`, nothing loads a kernel argument;
* the register budget of the prologue's tests holds.
"""
import os
import re

import pytest

from test_isa_waits import HIPCC, _device_asm, _kernel

KERNELS = [(xc, spec) for xc in (8, 16, 24, 32) for spec in (False, True)]
# Static instructions from the last ending block's record store to the kernel's end.  Before the gather moved: 207 without the speculative seed (XC = 24 and
# 32; 211 for XC = 8 and 16) and 348 - 353 with it, counted the same way.  Now 138 and 278 for every XC; the bound is that figure plus four instructions.
EXIT_BOUND = {False: 142, True: 282}
EXIT_BEFORE = {False: 207, True: 348}


def _instructions(body):
    lines = [ln.strip() for ln in body.split("\n")]
    return [ln for ln in lines if ln and not ln.startswith(";") and not ln.startswith(".")]


def _kernel_ins(xc, spec):
    body, meta = _kernel(_device_asm(), f"9slot_runxILi2ELi{xc}ELb0ELb{int(spec)}E")
    return body, meta, _instructions(body)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_nothing_gathers_behind_the_last_record_store(xc, spec):
    body, meta, ins = _kernel_ins(xc, spec)
    record = max(i for i, ln in enumerate(ins) if ln.startswith("global_store_byte"))
    assert ins[-1] == "s_endpgm", ins[-1]
    tail = ins[record:]
    assert not any(ln.startswith("v_bfe_u32") for ln in tail), (xc, spec, [ln for ln in tail if ln.startswith("v_bfe_u32")])
    assert sum(1 for ln in tail if ln.startswith("v_lshl_or_b32")) <= 2, (xc, spec, [ln for ln in tail if ln.startswith("v_lshl_or_b32")])
    # Kernel arguments are fetched with an immediate offset alone.  The one scalar load the stretch holds belongs to the column loop, whose last block stands
    # behind the last record store: the read-ahead of a third ending read's description, through the row pointer with a register offset.
    loads = [ln for ln in tail if ln.startswith("s_load")]
    assert all(re.match(r"s_load_dword s\d+, s\[\d+:\d+\], s\d+ offset:", ln) for ln in loads) and len(loads) <= 1, (xc, spec, loads)
    # the words of out_pos are not unpacked here either: a handful of scalar shifts, not one per slot
    assert sum(1 for ln in tail if ln.startswith("s_lshr_b32")) <= 2, (xc, spec, [ln for ln in tail if ln.startswith("s_lshr_b32")])
    assert len(tail) <= EXIT_BOUND[spec] and len(tail) <= EXIT_BEFORE[spec] - 60, (xc, spec, len(tail))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_the_gather_stands_under_the_prologues_wait(xc, spec):
    body, meta, ins = _kernel_ins(xc, spec)
    down = next(i for i, ln in enumerate(ins) if ln == "s_setprio 0")
    cells = next(i for i, ln in enumerate(ins) if ln.startswith("global_load_dwordx4"))
    last_request = max(i for i, ln in enumerate(ins[:down]) if re.match(r"global_load_dword v", ln))
    waits = [i for i, ln in enumerate(ins[:down]) if i > cells and ln.startswith("s_waitcnt") and "vmcnt" in ln]
    assert cells < last_request < waits[0], (xc, spec, cells, last_request, waits)
    # every slot from the first lane slot to the last grid slot: 24 extractions between the last request and the LAST wait in front of `s_setprio 0` ...
    gather = [i for i, ln in enumerate(ins) if last_request < i < waits[-1] and ln.startswith("v_bfe_u32")]
    assert len(gather) >= 6, (xc, spec, len(gather))
    # ... and, stronger, in front of the FIRST one: no loaded word is waited for before the gather has been issued
    early = [i for i in gather if i < waits[0]]
    assert len(early) == 24 and early == gather, (xc, spec, len(early), len(gather), waits[0])
    assert sum(1 for ln in ins[last_request:waits[0]] if ln.startswith("v_lshl_or_b32")) == 23, (xc, spec)
    # the table requests of the prologue stay in front of it (tests/test_xrun_prologue_isa.py counts them): the gather delays no request
    touches = [i for i, ln in enumerate(ins[:down]) if i > cells and ln.startswith("s_load_dword")]
    assert touches and max(touches) < gather[0], (xc, spec, max(touches), gather[0])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_the_register_budget_holds(xc, spec):
    body, meta, ins = _kernel_ins(xc, spec)
    assert meta["vgpr_count"] == 64 and meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (xc, spec, meta)
    assert "v_writelane" not in body and not re.search(r"\bscratch_", body), (xc, spec)
    # out_occ, L and the eight words of out_pos no longer travel through the loop (94 scalar registers in `<2, 24, false, false>` before, 85 - 90 over the eight kernels now)
    assert meta["sgpr_count"] <= 92, (xc, spec, meta)
