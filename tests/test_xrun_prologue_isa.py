"""No GPU needed: the request order of an X run's prologue, pinned on the cross-compiled assembly of `slot_runx<2, XC, false, SPEC>` for XC = 8, 16, 24, 32
(kernels_slots.h slot_runx_arguments / slot_runx_lds_core, DESIGN.md 4.1b "the prologue's request order", profiles/xrun_one_wait/).

A launch of 22 columns spent its first third before the first column, and the column loop cannot hide that part.  What the prologue is meant to be:

* ONE group of scalar loads through the kernel-argument pointer at the kernel's head and ONE wait behind it: every word the prologue, the loop's head and
  the exit use.  Behind that wait nothing loads through the kernel-argument pointer on the path the previous run's physical order takes (`in_identity`,
  one `global_load_dwordx4`); the general entry layout keeps one load of its own, the eight words of `in_pos`.
* exactly one wait for scalar data in front of the entering cells' request on that path;
* no wait for scalar data between the cells' request and `s_setprio 0`, and nothing but the loop's own requests at its head (the scalar table requests
  -- the sixteen Kr words of the first trip and the line touches -- stay behind the vector requests: moved in front of them they bought nothing);
* the flip of a halved run's mirrored group is four selects under one lane mask, not a select of the index with a dynamic extraction;
* 64 VGPRs (the ending block owns v56 .. v63), no spilled scalar.
"""
import os
import re

import pytest

from test_isa_waits import HIPCC, _device_asm, _kernel

IN_POS = 216 + 96   # sizeof(DevProblem) + offsetof(SlotRun, in_pos): the one kernel-argument load the general entry layout keeps
KERNELS = [(xc, spec) for xc in (8, 16, 24, 32) for spec in (False, True)]


def _instructions(body):
    lines = [ln.strip() for ln in body.split("\n")]
    return [ln for ln in lines if ln and not ln.startswith(";") and not ln.startswith(".")]


def _offset(ln):
    """The byte offset of a scalar load (`0xd8 + 160`, `40`, `0x198`)."""
    return sum(int(t, 0) for t in ln.split(",")[-1].split("+"))


def _prologue(xc, spec):
    body, meta = _kernel(_device_asm(), f"9slot_runxILi2ELi{xc}ELb0ELb{int(spec)}E")
    ins = _instructions(body)
    cells = [i for i, ln in enumerate(ins) if ln.startswith("global_load_dwordx4")]
    # the kernel-argument pointer is s[0:1] until something else is written there (in front of the cells' request only side blocks do: the path without `prev`)
    gone = next((i for i, ln in enumerate(ins) if i > cells[0] and (re.match(r"[sv]_\w+ s(0|1|\[0:1\]),", ln) or re.match(r"s_load_\w+ s\[0:\d+\],", ln))), len(ins))
    kargs = [i for i, ln in enumerate(ins[:gone]) if re.match(r"s_load_dword\w* \S+ s\[0:1\],", ln)]
    down = next(i for i, ln in enumerate(ins) if ln == "s_setprio 0")
    assert len(cells) == 1 and cells[0] < down, (xc, spec, cells, down)
    # the general entry layout: from its load of in_pos to the last of its four single-word loads of the cells
    general = [i for i in kargs if _offset(ins[i]) == IN_POS]
    assert len(general) == 1 and ins[general[0]].startswith("s_load_dwordx8"), (xc, spec, [ins[i] for i in general])
    singles = [i for i, ln in enumerate(ins) if general[0] < i < cells[0] and re.match(r"global_load_dword v", ln)]
    assert len(singles) == 4, (xc, spec, "the general entry layout loads four cells one by one", singles)
    return ins, meta, kargs, cells[0], down, (general[0], singles[-1])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_every_kernel_argument_is_requested_in_one_group_with_one_wait(xc, spec):
    ins, meta, kargs, cells, down, general = _prologue(xc, spec)
    waits = [i for i, ln in enumerate(ins) if ln.startswith("s_waitcnt") and "lgkmcnt" in ln]
    first = waits[0]
    assert ins[first] == "s_waitcnt lgkmcnt(0)", ins[first]
    late = [ins[i] for i in kargs if i > first and i != general[0]]
    assert not late, (xc, spec, "loaded through the kernel-argument pointer behind the first wait", late)
    head = [i for i in kargs if i < first]
    assert len(head) >= 10 and head == list(range(head[0], head[0] + len(head))), (xc, spec, "the group is not one run of scalar loads", head)
    # the words of the loop's head and of the exit are in the group: cur / score_out / pack behind prev, P.bt, P.slot_rows, out_pos
    offsets = {_offset(ins[i]) for i in head}
    assert {0x28, 0x70, 0x88, 216 + 128, 408, 408 + 8, 408 + 16, 408 + 24} <= offsets, (xc, spec, sorted(hex(o) for o in offsets))
    # exactly one wait for scalar data in front of the entering cells' request on the in_identity path
    on_path = [i for i in waits if i < cells and not general[0] <= i <= general[1]]
    assert on_path == [first], (xc, spec, [ins[i] for i in on_path])
    # the younger half raises its priority while the group travels: between the group's last load and the wait
    up = next(i for i, ln in enumerate(ins) if ln == "s_setprio 1")
    assert head[-1] < up < first, (xc, spec, head[-1], up, first)
    # the cells' address is the first vector memory operation behind the wait on that path, and no scalar load stands in between
    between = [ln for i, ln in enumerate(ins[first:cells]) if not general[0] <= first + i <= general[1]]
    assert not any(re.match(r"s_load|global_|ds_|buffer_", ln) for ln in between), (xc, spec, between)
    # ... nor the tables' address arithmetic (64-bit scalar adds, the row products): the request does not need it
    assert not any(re.match(r"s_addc_u32|s_lshl_b64|s_mul_i32|s_mul_hi_u32", ln) for ln in between), (xc, spec, "table-address arithmetic in front of the entering cells' request")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_nothing_waits_for_scalar_data_between_the_entering_cells_and_the_loop(xc, spec):
    """(The scalar table requests in FRONT of the lane parts' vector loads were measured and not kept -- profiles/xrun_one_wait/experiments_not_kept.md: the
    wait at the loop's head holds a wave for 41 - 49 cycles only.  They stand behind every vector request, touches included, and nothing waits for them
    before the loop's head.)"""
    ins, meta, kargs, cells, down, general = _prologue(xc, spec)
    lane_parts = [i for i, ln in enumerate(ins) if cells < i < down and re.match(r"global_load_dword v", ln)]
    assert len(lane_parts) == xc + 3, (xc, spec, len(lane_parts))   # (the lane parts of XC columns, the workgroup's and the wave's part, the lanes' tie parities)
    kr = [i for i, ln in enumerate(ins) if cells < i < down and ln.startswith("s_load_dwordx16")]
    touches = [i for i, ln in enumerate(ins) if cells < i < down and re.match(r"s_load_dword s\d+, s\[\d+:\d+\], (64|128|192|256|320|384|448|512)$", ln)]
    assert len(kr) == 1 and len(touches) == (4 if xc <= 8 else 8) + (2 if xc > 24 else 0) + 2, (xc, spec, kr, len(touches))
    assert not any(ln.startswith("s_waitcnt") and "lgkmcnt" in ln for ln in ins[cells:down]), (xc, spec, "a wait for scalar data between the cells' request and s_setprio 0")
    # the loop's head: its own requests only -- the LDS line of the first trip and ONE wait in front of the first column
    first_column = next(i for i, ln in enumerate(ins) if re.match(r"v_sad_u32 v\d+, v\d+, s\d+, v\d+", ln))
    head = ins[down:first_column]
    assert not any(ln.startswith("s_load") and "s[0:1]" in ln for ln in head[:12]), (xc, spec, head[:12])
    assert sum(1 for ln in head if ln.startswith("ds_read_b128")) >= 1 and not any(ln.startswith("global_load") for ln in head), (xc, spec, head)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("xc,spec", KERNELS)
def test_the_flip_is_four_selects_and_the_register_budget_holds(xc, spec):
    ins, meta, kargs, cells, down, general = _prologue(xc, spec)
    last_wait = max(i for i, ln in enumerate(ins[:down]) if ln.startswith("s_waitcnt") and "vmcnt" in ln)
    tail = ins[last_wait:down]
    selects = [ln for ln in tail if ln.startswith("v_cndmask")]
    assert len(selects) <= 4, (xc, spec, selects)
    masks = {ln.split(",")[-1].strip() for ln in selects if re.match(r"v_cndmask_b32_e64 v\d+, v\d+, v\d+, s\[\d+:\d+\]$", ln)}
    assert len([ln for ln in selects if re.match(r"v_cndmask_b32_e64 v\d+, v\d+, v\d+, s\[", ln)]) == 4 and len(masks) == 1, (xc, spec, selects)
    # the select of an index: v_cmp_eq against 1, 2, 3 -- wait states -- v_cndmask, over and over
    assert not any(re.match(r"v_cmp_eq_u32\w* (vcc|s\[\d+:\d+\]), [123], v\d+", ln) for ln in tail), (xc, spec, tail)
    assert sum(1 for ln in tail if ln.startswith("s_nop")) <= 1, (xc, spec, [ln for ln in tail if ln.startswith("s_nop")])
    assert meta["vgpr_count"] == 64 and meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (xc, spec, meta)
    body, _ = _kernel(_device_asm(), f"9slot_runxILi2ELi{xc}ELb0ELb{int(spec)}E")
    assert "v_writelane" not in body and not re.search(r"\bflat_", body), (xc, spec)
