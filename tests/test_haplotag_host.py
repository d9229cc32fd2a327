"""CPU: haplotagging (whatshap_amd.haplotag) on one host thread of the debug library against what the reference's
prepare_haplotag_information recorded for every case of tests/haplotag_cases.py -- identical in every field: the assignment of every
representation, the BX lists in order, n_multiple_phase_sets, primary_info_by_repr; a ValueError where the reference raises."""
import numpy as np
import pytest

import haplotag_cases as hc
from whatshap_amd import haplotag as ht

GOLDEN = {c["spec"]["name"]: c for c in hc.load_golden()["cases"]}
SPECS = {s["name"]: s for s in hc.all_specs()}
# the reference's exception -> what it means here (ploidy 17 does not raise there: the limit is this library's)
REFERENCE_ERRORS = {"error_ploidy_1": "IndexError", "error_ploidy_17": None, "error_unknown_position": "KeyError", "error_unphased_position": "KeyError",
                    "error_allele_2": "AssertionError", "error_allele_negative": "AssertionError"}


def test_every_spec_is_recorded_and_generates_the_recorded_input():
    assert sorted(GOLDEN) == sorted(SPECS)
    for name, spec in SPECS.items():
        assert hc.input_sha256(hc.materialize(spec)) == GOLDEN[name]["input_sha256"], name
    assert sum(c.get("multi_read_groups", 0) for c in GOLDEN.values()) >= 20
    assert {name: GOLDEN[name]["raises"] for name in REFERENCE_ERRORS} == REFERENCE_ERRORS
    assert all(c["raises"] is None for name, c in GOLDEN.items() if name not in REFERENCE_ERRORS)
    assert {s["ploidy"] for s in SPECS.values() if not s["expect_error"]} == {2, 3, 4, 6, 8, 16}


@pytest.mark.parametrize("name", [n for n, s in SPECS.items() if not s["expect_error"]])
def test_host_twin_equals_the_reference(name):
    spec = SPECS[name]
    stats = []
    got = hc.canonical(ht.prepare_haplotag_information(*hc.call_args(spec, hc.materialize(spec)), host=True, stats=stats))
    want = GOLDEN[name]["results"]
    assert got["n_multiple_phase_sets"] == want["n_multiple_phase_sets"]
    assert got["reads"] == want["reads"]
    assert got["bx"] == want["bx"]
    assert got["primary"] == want["primary"]
    assert all(s["launches"] == 0 for s in stats)


@pytest.mark.parametrize("name", [n for n, s in SPECS.items() if s["expect_error"]])
def test_errors(name):
    spec = SPECS[name]
    with pytest.raises(ValueError) as e:
        ht.prepare_haplotag_information(*hc.call_args(spec, hc.materialize(spec)), host=True)
    if name == "error_ploidy_17":
        assert "16" in str(e.value)


def test_native_validation_of_arrays():
    """The same errors from the array-level call, where the native library finds them (nothing is launched: the device is never opened)."""
    ok = dict(variant_position=[10, 20], variant_phaseset=[1, 1], variant_phasing=[[0, 1], [1, 0]], read_ptr=[0, 2], entry_position=[10, 20], entry_allele=[0, 1],
              entry_quality=[5, 6], read_start=[3], read_repr=[0])
    assert ht.haplotag_batch([ht.HaplotagProblem(2, **ok)], host=True)[0].haplotype.tolist() == [0]
    for change, match in ((dict(entry_position=[10, 15]), "unknown position"), (dict(entry_allele=[0, 2]), "allele 2"), (dict(entry_allele=[0, 300]), "allele"),
                          (dict(variant_position=[10, 10]), "twice"), (dict(read_repr=[4]), "dense")):
        with pytest.raises(ValueError, match=match):
            ht.haplotag_batch([ht.HaplotagProblem(2, **dict(ok, **change))], host=True)
        with pytest.raises(ValueError, match=match):   # the product library validates before it looks for a device
            ht.haplotag_batch([ht.HaplotagProblem(2, **dict(ok, **change))])
    for ploidy in (1, 17, 0, -2):
        with pytest.raises(ValueError):
            ht.HaplotagProblem(ploidy, **ok)
    with pytest.raises(ValueError, match="int32"):
        ht.HaplotagProblem(2, **dict(ok, entry_quality=[5, 1 << 31]))


def test_array_level_call_agrees_with_the_reference_signature_call():
    for name in ("mixed_p4", "linked_short_reads", "linked_two_samples", "representations_linked", "tie_heavy_p3"):
        spec = SPECS[name]
        data = hc.materialize(spec)
        _, reads, n_multiple, _ = ht.prepare_haplotag_information(*hc.call_args(spec, data), host=True)
        table, samples, reader = hc.CaseTable(data), data["sample_order"], hc.CaseReader(data)
        problems = []
        for sample in samples:
            info, variants = ht.get_variant_information(table, sample)
            problems.append(ht.HaplotagProblem.from_reads(info, reader.read(table.chromosome, variants, sample)[0], spec["ploidy"], spec["ignore_linked_read"],
                                                          spec["cutoff"]))
        results = ht.haplotag_batch(problems, host=True)
        merged = {}
        for p, res in zip(problems, results):
            for r in np.flatnonzero(res.haplotype >= 0).tolist():
                merged[p.reprs[int(p.read_repr[r])]] = (int(res.haplotype[r]), int(res.quality[r]), int(res.phaseset[r]))
        assert merged == reads
        assert sum(res.n_multiple_phase_sets for res in results) == n_multiple


def test_reader_arguments_and_representation_hook():
    spec = SPECS["two_samples"]
    data = hc.materialize(spec)
    args = hc.call_args(spec, data)
    seen = []

    def representation(read, as_primary=False):
        seen.append(as_primary)
        r = ht.read_representation(read, as_primary)
        return (r.read_name, r.chromosome, r.is_supplementary, r.sub_alignment_id)

    _, reads, _, primary = ht.prepare_haplotag_information(*args, supplementary_strategy="copy-primary", representation=representation,
                                                           host=True)
    assert all(isinstance(k, tuple) for k in list(reads) + list(primary)) and True in seen and False in seen
    want = {tuple(r[:4]): tuple(r[4:]) for r in GOLDEN["two_samples"]["results"]["reads"]}
    assert reads == want
    # the reader was asked per sample for the chromosome's non-homozygous phased variants, regions passed through
    assert [(c[0], c[2], c[3]) for c in args[2].calls] == [(hc.CHROMOSOME, "s0", None), (hc.CHROMOSOME, "s1", None)]
    assert args[2].calls[0][1] == data["positions"]


def test_stats_of_the_host_twin_on_a_mixed_problem():
    """Class counts follow the group sizes (1 .. 64, 65 .. 4096, more); the many-phase-set count is the groups with more than 4 phase sets."""
    lengths = [0, 1, 64, 65, 4096, 4097, 3, 0, 200]
    p = hc.array_problem(2, lengths, seed=3, n_phasesets=6, n_variants=6000, window=6000)
    stats = []
    res = ht.haplotag_batch([p], host=True, stats=stats)[0]
    s = stats[0]
    assert (s["n_reads"], s["n_groups"], s["n_entries"]) == (9, 9, sum(lengths))
    assert (s["groups_class_a"], s["groups_class_b"], s["groups_class_c"]) == (3, 3, 1)
    assert s["groups_many_phase_sets"] == 5 and s["n_multiple_phase_sets"] == res.n_multiple_phase_sets >= 5
    assert s["launches"] == 0 and s["n_assigned"] == int((res.haplotype >= 0).sum())
