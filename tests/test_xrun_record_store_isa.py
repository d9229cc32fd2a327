"""No GPU needed: the backtrace record store of the X runs' ending blocks, pinned on the cross-compiled assembly (kernels_slots.h SLOTX_ENDING_ASM /
SLOTX8_ENDING_ASM, SLOTX_REC_POLICY; DESIGN.md 4.1b "the record store is non-temporal"; profiles/record_pairs/).

Nothing reads the record before the backtrace, so its lines have no business in the L2 flush between two dependent launches.  What the kernels are meant to do:

* every ending block stores the thread's record byte exactly once, with the `nt` policy and with no other one (`sc1` and `sc0 sc1` were measured slower);
* the offset register advances right behind the store, by the workgroup's size (a scalar), as before;
* the policy costs no register: the budgets of the headline kernels are what they were.
"""
import os
import re

import pytest

from test_isa_waits import HIPCC, _device_asm, _kernel

# (mangled fragment, `s_cmp_lt_u32 ..., N` that follows an ending block's opening s_bfe_u32, vgpr_count, highest sgpr_count, scalar spills) -- the register
# figures are the parent's own for these kernels
KERNELS = [
    ("9slot_runxILi2ELi24ELb0ELb0E", 8, 64, 85, 0),
    ("9slot_runxILi2ELi32ELb0ELb0E", 8, 64, 86, 0),
    ("9slot_runxILi2ELi0ELb0ELb0E", 8, 64, 106, 5),
    ("11slot_groupxILi2ELb0E", 8, 64, 97, 0),
    ("11slot_groupxILi3ELb0E", 9, 64, 92, 0),
]


def _instructions(body):
    lines = [ln.strip() for ln in body.split("\n")]
    return [ln for ln in lines if ln and not ln.startswith(";") and not ln.startswith(".")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("frag,first_wave_slot,vgprs,sgprs,spills", KERNELS)
def test_every_ending_block_stores_its_record_byte_once_and_non_temporal(frag, first_wave_slot, vgprs, sgprs, spills):
    body, meta = _kernel(_device_asm(), frag)
    ins = _instructions(body)
    blocks = [i for i, ln in enumerate(ins) if ln.startswith("s_bfe_u32") and re.match(rf"s_cmp_lt_u32 s\d+, {first_wave_slot}$", ins[i + 1])]
    stores = [i for i, ln in enumerate(ins) if ln.startswith("global_store_byte")]
    assert len(blocks) >= 8 and len(stores) == len(blocks), (frag, len(blocks), len(stores))
    # one store per block: block, store, block, store, ...
    order = sorted([(i, "b") for i in blocks] + [(i, "s") for i in stores])
    assert [k for _, k in order] == ["b", "s"] * len(blocks), frag
    for i in stores:
        assert re.match(r"global_store_byte v\d+, v\d+, s\[\d+:\d+\] nt$", ins[i]), (frag, ins[i])
        # the offset of the next ending read's byte: + threads, a scalar
        assert re.match(r"v_add_u32_e32 v\d+, s\d+, v\d+$", ins[i + 1]), (frag, ins[i + 1])
        assert ins[i].split()[1] == ins[i + 1].split()[1] == ins[i + 1].split()[3] + ",", (frag, ins[i], ins[i + 1])
    # no other store of the kernel asks for a cache policy: the exit column is what the next launch reads
    # (a shared launch's pointers come from memory: its exit stores are flat ones)
    others = [ln for ln in ins if re.match(r"(global|flat)_store_(?!byte)", ln)]
    assert others and not any(re.search(r"\b(nt|sc0|sc1)\b", ln) for ln in others), (frag, [ln for ln in others if re.search(r"\b(nt|sc0|sc1)\b", ln)])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("frag,first_wave_slot,vgprs,sgprs,spills", KERNELS)
def test_the_policy_costs_no_register(frag, first_wave_slot, vgprs, sgprs, spills):
    body, meta = _kernel(_device_asm(), frag)
    assert meta["vgpr_count"] == vgprs and meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (frag, meta)
    assert meta["sgpr_count"] <= sgprs and meta["sgpr_spill_count"] <= spills, (frag, meta)
