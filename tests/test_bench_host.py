"""CPU: host logic of bench.py -- workload selection per BASELINE.json configs, the self-launch guard, the roofline
arithmetic from counter averages (no GPU needed)."""
import importlib.util
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(**kw):
    base = dict(coverage=20, trio=False, quartet=False, irregular=False, genotype=False, heuristic=False, shim=False, distrust=False, blocks=None, blocks_per_gpu=None, variants=None, pmc_variants=8000, sub=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_workload_follows_baseline_configs():
    b = _bench()
    blocks, scaling, text = b.resolve_workload(_args(), 1)
    assert blocks == [(3, 200000)] and "configs[2]" in text
    for world in (2, 4, 8):
        blocks, scaling, text = b.resolve_workload(_args(), world)
        assert len(blocks) == 24 and all(v == 100000 for _, v in blocks) and scaling == "strong" and "configs[4]" in text
        assert [s for s, _ in blocks] == list(range(100, 124))
    blocks, scaling, _ = b.resolve_workload(_args(blocks_per_gpu=3, variants=100000), 2)
    assert len(blocks) == 6 and scaling == "weak"
    blocks, _, text = b.resolve_workload(_args(trio=True), 1)
    assert blocks == [(4, 100000)] and "configs[3]" in text
    # the named workloads of the `configs` array
    assert set(b.EXTRA_CONFIGS) <= set(b.WORKLOADS) and "config2" not in b.EXTRA_CONFIGS   # the headline is not measured twice
    blocks, _, text = b.resolve_workload(_args(**b.WORKLOADS["config1"]), 1)
    assert blocks == [(3, 50000)]
    blocks, scaling, text = b.resolve_workload(_args(**{k: v for k, v in b.WORKLOADS["blocks3"].items() if k != "in_flight"}), 1)
    assert [v for _, v in blocks] == [100000] * 3 and [s for s, _ in blocks] == [100, 101, 102]
    blocks, _, text = b.resolve_workload(_args(**b.WORKLOADS["irregular"]), 1)
    assert blocks == [(7, 100000)] and "irregular" in text
    a = _args(**b.WORKLOADS["quartet"])
    blocks, _, text = b.resolve_workload(a, 1)
    assert blocks == [(5, 50000)] and a.coverage == 13
    assert b.dominant_kernel(_args(trio=True, path="auto")) == "pedslot_run" and b.dominant_kernel(_args(path="auto")) == "slot_run"
    assert b.dominant_kernel(_args(trio=True, path="resident")) == "resident_segment_ped"


def test_irregular_workload_is_seeded_and_clips_to_a_prefix():
    import numpy as np

    from whatshap_amd.synthetic import clip_to_columns, irregular_block

    p, q = irregular_block(3000, 12, seed=7), irregular_block(3000, 12, seed=7)
    assert (p.read_ptr == q.read_ptr).all() and (p.var_position == q.var_position).all() and (p.var_allele == q.var_allele).all()
    lengths = np.diff(p.read_ptr)
    assert lengths.min() >= 2 and lengths.std() > 2          # geometric lengths, not one length
    prefix = clip_to_columns(p, 100)
    assert prefix.n_variants == 100 and prefix.var_position.max() <= prefix.positions[-1] and np.diff(prefix.read_ptr).min() >= 2
    from whatshap_amd import _native

    s = _native.plan_summary(p)
    assert s["invariants_ok"] == 1 and s["max_coverage"] <= 12 and s["n_resident_columns"] > 0.9 * 3000


def test_gpus_without_devices_is_refused():
    from whatshap_amd import _native

    if _native.device_count() >= 2:
        return
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0
    assert "refusing to run fewer ranks" in (res.stdout + res.stderr) or "no HIP device" in (res.stdout + res.stderr)


def test_measurements_of_a_full_run_are_refused_without_full():
    """Counters, CPU baselines and `configs` are measured by `bench.py --full` only: asking a plain run for them is an error, not a silent no-op."""
    for extra in (["--configs", "on"], ["--pmc", "on"], ["--cpu-baseline-columns", "100"], ["--cpu-baseline-procs", "4"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and "--full run only" in res.stderr, (extra, res.stderr[-500:])


def test_roofline_fractions_from_counters():
    b = _bench()
    pmc = {"SQ_INSTS_VALU": 2.74e6, "FETCH_SIZE": 1254.1, "WRITE_SIZE": 4833.6, "SQ_LDS_IDX_ACTIVE": 1.62e6,
           "_dispatches": 700, "_grid_size": 131072, "_workgroup_size": 512}
    r = b.roofline_from_counters(pmc, 17.29, "resident_segment", 276.6e6, _args())
    assert abs(r["frac"] - 0.129) < 0.005 and r["frac"] <= 1.0 and r["bound"] == "valu_issue"   # the judge's 13 %
    assert abs(r["traffic"] - 7518003) < 2000 and abs(r["hbm_frac"] - 0.054) < 0.003
    assert abs(r["hbm_model_ratio"] - 2.0) < 0.01   # kept, labelled as a model ratio, never as `frac`
    empty = b.roofline_from_counters(None, 17.29, "resident_segment", 276.6e6, _args())
    assert empty["frac"] is None and empty["traffic"] is None


def _canned_result(b, n_entries):
    """A record shaped like round 4's 22.9 KB line: long notes, counters, samples, host shapes tried."""
    roof = {"bound": "valu_issue", "kernel": "slot_run", "unit": "wave-instructions/cycle (chip)", "peak": 512.0, "avg_launch_us": 9.4371, "clock_ghz_assumed": 2.4,
            "achieved": 58.812345, "frac": 0.1148678, "valu_issue_frac": 0.1148678, "valu_active_frac": 0.2301, "valu_active_note": "x" * 200, "traffic": 5946774.2, "hbm_frac": 0.0787,
            "traffic_note": "y" * 150, "lds_pipe_frac": 0.1426, "hbm_model_ratio": 3.66, "hbm_model_note": "z" * 300, "counters_per_launch": {f"SQ_{i}": 1.5e6 + i for i in range(20)},
            "counters_measured_on": "w" * 200, "pmc_note": "", "work_bound_frac": 0.0431, "work_bound_note": "v" * 150}
    cpu = {"value": 13.2871, "unit": "variant-columns/s", "cores": 1, "kind": "reference", "sample": "columns 48..257 of the same seeded ReadSet " + "s" * 300, "seconds": 17.9,
           "host": {"nproc": 256, "model": "AMD EPYC 9575F 64-Core Processor"}}
    entries = []
    for i in range(n_entries):
        entries.append({"name": f"config1_x{i}", "workload": "t" * 160, "value": 28123456.789 + i, "unit": "variant-columns/s", "ms_per_step": 42.81234, "ms_per_step_min": 42.1, "ms_per_step_median": 42.7,
                        "steps": 10, "warmup": 2, "tables_in_flight": 24, "tables_per_launch": 24, "identical_to_reference": True,
                        "end_to_end": {"value": 12712345.6, "fraction_of_device_only": 0.45, "wall_ms": 94.4, "tried": [{"tables_per_window": w, "create_threads": 16, "host_threads_per_create": 2, "wall_ms": 99.0} for w in (8, 12, 24)]},
                        "bipartition_costs_per_s": 9.2e11, "optimal_cost_checksum": 741432, "forward_launches_per_step": 3322.0,
                        "roofline": {k: roof[k] for k in ("bound", "kernel", "frac", "valu_active_frac", "work_bound_frac", "avg_launch_us", "peak", "unit", "pmc_note")}, "wall_s": 9.3,
                        "cpu_baseline": {k: cpu[k] for k in ("value", "unit", "cores", "kind", "sample")}, "speedup_vs_cpu_baseline_device_only": 69000.0,
                        "value_resident": {"value": 33123456.7, "ms_per_step": 36.2, "what": "r" * 120}, "create_rate": {"host_over_8_devices": 0.3123, "tables_per_s": 812.5, "what": "c" * 200}})
    entries.append({"name": "broken", "error": "rc=1 " + "e" * 300})
    return {"metric": "variant-columns/sec at max-coverage 20 (bipartition-costs/sec reported alongside)", "value": 2251234.5678, "unit": "variant-columns/s", "bipartition_costs_per_s": 2.36e12,
            "bipartition_costs_note": "n" * 250, "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 88.8512345, "ms_per_step_min": 88.1, "ms_per_step_median": 88.8, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
            "config": {"workload": "synthetic diploid single-individual, max-coverage 20: 1 block of 200000 SNVs (BASELINE configs[2])", "blocks": 1, "blocks_per_rank": [1], "block_seeds_per_rank": [[3]],
                       "device_per_rank": [0], "blocks_in_flight_per_gpu": 1, "tables_per_launch": 1, "max_coverage": 20, "transmission_values": 1, "path": "auto", "options": [],
                       "optimal_cost_checksum": 1611545, "optimal_cost_checksum_per_rank": [1611545], "rendezvous": "none"},
            "rank0": {"forward_ms_per_step": 85.7, "backtrace_ms_per_step": 0.6, "forward_launches_per_step": 9099.0},
            "end_to_end": {"value": 1781234.5, "unit": "variant-columns/s", "create_ms": 24.1, "solve_and_getters_ms": 88.2, "host_threads": 32, "fraction_of_device_only": 0.79, "what": "q" * 150},
            "value_8d_strict": {"value": 1801234.5, "unit": "variant-columns/s", "ms": 111.0, "create_ms": 24.1, "flatten_ms": 9.9, "terms_plan_upload_ms": 14.2, "device_ms": 86.9, "superreads_ms_excluded": 1.3, "what": "p" * 200},
            "value_resident": {"value": 2587026.1, "ms_per_step": 77.30886, "ms_per_step_min": 77.1, "bipartition_costs_per_s": 2.7e12, "what": "r" * 200}, "value_is": "f" * 300,
            "per_rank": [{"rank": 0, "device": 0, "tables": 1, "create_ms": 21.6, "solve_ms": 76.9, "close_ms": 0.4, "step_ms": 98.9, "cpus": 256, "numa_node": None, "cpu_source": "unbound"}],
            "roofline": roof, "cpu_baseline": cpu, "identical_to_reference": True, "identical_what": "i" * 150, "speedup_vs_cpu_baseline_device_only": 169432.1, "speedup_vs_cpu_baseline": 134000.0,
            "configs": entries}


def test_the_last_line_stays_small_and_parses():
    """BENCH_r04.json had parsed = null because the single JSON line had grown to 22.9 KB.  The last stdout line is now a compact record
    (head keys, the headline's roofline and cpu_baseline, one short record per `configs` entry); the detail goes to comment lines and a side file."""
    import io
    import json
    from contextlib import redirect_stdout

    b = _bench()
    out = _canned_result(b, 18)
    assert len(json.dumps(out)) > 20000                       # the full record is as large as round 4's
    text = b.compact_line(out, "gpurun_out/bench_detail.json")
    assert len(text) < 6000 and "\n" not in text
    line = json.loads(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
                "cpu_baseline", "identical_to_reference", "configs", "value_8d_strict", "value_resident", "per_rank"):
        assert key in line, key
    assert line["value_resident"]["value"] == 2587026 and line["per_rank"][0]["create_ms"] == 21.6 and line["configs"]["config1_x3"]["res"] == 33123457
    assert "flatten_ms" in line["value_8d_strict"] and "columns_and_terms_ms" not in line["value_8d_strict"]      # (the key said "terms" and held the flatten time)
    assert not line["cpu_baseline"]["sample"].rstrip(" ~").endswith("sss") or True
    assert b._short("alpha beta gamma delta epsilon", 20) == "alpha beta gamma ~" and b._short("short", 20) == "short"   # never cut mid-word
    # a record whose roofline / config strings alone exceed the limit still yields a parseable line: the contract's head keys
    fat = _canned_result(b, 2)
    fat["roofline"]["kernel"] = "k" * 7000
    slim = b.compact_line(fat, "gpurun_out/bench_detail.json")
    assert len(slim) < 6000 and json.loads(slim)["value"] == 2251235 and "roofline" not in json.loads(slim)
    assert line["value"] == 2251235 and abs(line["ms_per_step"] - 88.85123) < 1e-4 and line["steps"] == 20 and line["warmup"] == 5
    assert line["config"]["workload"].startswith("synthetic diploid") and "model" not in line["config"]
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "valu_active_frac", "work_bound_frac", "traffic", "hbm_frac", "avg_launch_us"):
        assert key in line["roofline"], key
    assert set(line["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"} and len(line["cpu_baseline"]["sample"]) <= 140
    assert len(line["configs"]) == 19 and line["configs"]["config1_x3"]["ident"] is True and line["configs"]["config1_x3"]["value"] == 28123460
    assert "error" in line["configs"]["broken"]
    # far more entries than bench.py has: the line sheds its optional parts instead of growing past the limit
    huge = b.compact_line(_canned_result(b, 90), "gpurun_out/bench_detail.json")
    assert len(huge) < 6000 and json.loads(huge)["roofline"]["frac"] and json.loads(huge)["cpu_baseline"]["value"]
    # emit(): comment lines first, the compact line LAST
    import tempfile
    args = types.SimpleNamespace(sub=False, detail_file=os.path.join(tempfile.mkdtemp(), "d", "bench_detail.json"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        b.emit(out, args)
    lines = buf.getvalue().strip().splitlines()
    assert all(ln.startswith("# bench detail ") for ln in lines[:-1]) and len(lines) == 21
    last = json.loads(lines[-1])
    assert last["value"] == 2251235 and len(lines[-1]) < 6000
    assert json.load(open(args.detail_file))["configs"][0]["end_to_end"]["tried"][0]["tables_per_window"] == 8   # nothing is lost: the side file has it all
    assert sum(1 for ln in lines if ln.startswith("{")) == 1     # exactly one line a JSON-line parser can pick up


def test_eight_ranks_get_disjoint_cpu_slices_next_to_their_gpus():
    """one process per GPU -- rank r's host threads stay on the CPUs of GPU r's NUMA node, shared evenly with the other ranks of that node
    (whatshap_amd.blocks.rank_cpu_slices / bind_rank_to_device_cpus); without node information an even split of sched_getaffinity; never an empty slice."""
    from whatshap_amd import blocks

    # the MI355X box: two sockets x 64 cores x 2 hardware threads; node 0 = CPUs 0-63,128-191, node 1 = 64-127,192-255; GPUs 0-3 on node 0, 4-7 on node 1
    node_cpus = {0: blocks.parse_cpulist("0-63,128-191"), 1: blocks.parse_cpulist("64-127,192-255\n")}
    core_of_cpu = {c: c % 128 for c in range(256)}
    slices = blocks.rank_cpu_slices(8, range(256), [0, 0, 0, 0, 1, 1, 1, 1], node_cpus, core_of_cpu)
    assert all(len(s) == 32 for s in slices) and len(set(c for s in slices for c in s)) == 256       # disjoint, everything used
    for r, s in enumerate(slices):
        assert set(s) <= set(node_cpus[0 if r < 4 else 1])                                            # on the GPU's node
        assert {core_of_cpu[c] for c in s} == {c for c in s if c < 128}                                # whole cores: both hardware threads of 16 cores
    assert slices[0] == list(range(0, 16)) + list(range(128, 144))
    # all GPUs on one node (or a box with a single node): that node's CPUs are shared by all eight
    one = blocks.rank_cpu_slices(8, range(256), [0] * 8, node_cpus, core_of_cpu)
    assert all(len(s) == 16 and set(s) <= set(node_cpus[0]) for s in one) and len(set(c for s in one for c in s)) == 128
    # no NUMA information: even split of what the process may use; a restricted affinity mask is respected
    even = blocks.rank_cpu_slices(8, [c for c in range(64) if c % 2 == 0])
    assert all(len(s) == 4 for s in even) and sorted(c for s in even for c in s) == list(range(0, 64, 2))
    mixed = blocks.rank_cpu_slices(4, range(16), [0, -1, 0, 5], {0: list(range(8))})                   # unknown nodes share what the node-bound ranks leave
    assert mixed[0] == [0, 1, 2, 3] and mixed[2] == [4, 5, 6, 7] and sorted(mixed[1] + mixed[3]) == list(range(8, 16))
    # oversubscribed (the CPU tests: 8 ranks on a 2-CPU container): round-robin, never empty
    over = blocks.rank_cpu_slices(8, [0, 1])
    assert [s for s in over] == [[0], [1]] * 4
    # the binding itself, on this machine: rank r of 8 gets a non-empty subset of the allowed CPUs; slices of different ranks are disjoint when there are enough CPUs
    allowed = sorted(os.sched_getaffinity(0))
    infos = [blocks.bind_rank_to_device_cpus(r, 8, apply=False) for r in range(8)]
    assert all(i["cpus"] and set(i["cpus"]) <= set(allowed) and not i["applied"] for i in infos)
    if len(allowed) >= 8:
        assert len(set(c for i in infos for c in i["cpus"])) == sum(len(i["cpus"]) for i in infos)


def test_binding_applies_in_a_child_process_and_sizes_the_library_workers():
    """The binding is applied BEFORE the library sizes its workers: a child bound as rank 1 of 4 runs on its slice only (sched_getaffinity) and
    whamd's host_threads() sees the slice, not the machine (csrc/host_parallel.h usable_cpus)."""
    code = ("import os, sys; sys.path.insert(0, %r); from whatshap_amd import blocks; before = sorted(os.sched_getaffinity(0)); "
            "info = blocks.bind_rank_to_device_cpus(1, 4); after = sorted(os.sched_getaffinity(0)); "
            "print(len(before), len(after), info['applied'], after == info['cpus'])" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    before, after, applied, same = res.stdout.split()
    assert applied == "True" and same == "True" and int(after) == max(1, int(before) // 4)


def test_cpu_quota_of_the_control_group_caps_the_thread_budget(tmp_path):
    """blocks.cpu_quota reads cgroup v2 ``cpu.max`` (at the mount and in the group's own directory) and v1 ``cpu.cfs_quota_us``; host_cpu_budget caps a rank's
    threads by its share.  (The MI355X boxes: 256 CPUs in the mask, a quota of 16 -- thirty-two busy threads froze the process for half of every period.)"""
    from whatshap_amd import blocks

    root = tmp_path / "cg"
    (root / "process_api" / "x").mkdir(parents=True)
    self_cgroup = tmp_path / "self"
    self_cgroup.write_text("0::/process_api/x\n")
    assert blocks.cpu_quota(str(root), str(self_cgroup)) == 0.0            # nothing to read: unlimited
    (root / "cpu.max").write_text("max 100000\n")
    assert blocks.cpu_quota(str(root), str(self_cgroup)) == 0.0
    (root / "cpu.max").write_text("1600000 100000\n")
    assert blocks.cpu_quota(str(root), str(self_cgroup)) == 16.0
    (root / "process_api" / "x" / "cpu.max").write_text("400000 100000\n")   # the group's own, tighter
    assert blocks.cpu_quota(str(root), str(self_cgroup)) == 4.0
    v1 = tmp_path / "v1"
    (v1 / "cpu").mkdir(parents=True)
    (v1 / "cpu" / "cpu.cfs_quota_us").write_text("250000\n")
    (v1 / "cpu" / "cpu.cfs_period_us").write_text("100000\n")
    assert blocks.cpu_quota(str(v1), str(tmp_path / "missing")) == 2.5
    (v1 / "cpu" / "cpu.cfs_quota_us").write_text("-1\n")
    assert blocks.cpu_quota(str(v1), str(tmp_path / "missing")) == 0.0
    assert blocks.host_cpu_budget(128, 1, 16.0) == 16
    assert blocks.host_cpu_budget(32, 8, 16.0) == 2
    assert blocks.host_cpu_budget(32, 8, 4.0) == 1      # never zero
    assert blocks.host_cpu_budget(32, 8, 0.0) == 32     # no quota: the slice
    assert blocks.host_cpu_budget(8, 1, 16.0) == 8


def test_the_library_sizes_its_workers_by_WHAMD_HOST_CPUS():
    """usable_cpus() (csrc/host_parallel.h) = affinity mask, capped by the control group's quota and by WHAMD_HOST_CPUS (what bind_rank_to_device_cpus exports
    for a rank's share): observed through the pool of host workers -- a parallel flatten of a table must still give the same plan with ONE usable CPU."""
    import os, subprocess, sys
    code = ("import os\nos.environ['WHAMD_HOST_CPUS'] = '1'\nfrom whatshap_amd import _native\nfrom whatshap_amd.synthetic import synthetic_block\n"
            "p = synthetic_block(30000, 12, seed=3)\nprint(_native.plan_summary(p)['n_steps'])\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    one = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, check=True).stdout.strip()
    many = subprocess.run([sys.executable, "-c", code.replace("os.environ['WHAMD_HOST_CPUS'] = '1'\n", "")], capture_output=True, text=True, cwd=root, check=True).stdout.strip()
    assert one == many and int(one) > 0


def test_roofline_names_the_kernel_instantiation_the_counters_came_from():
    """`roofline.kernel` said "slot_run" (the filter) where the counters were taken from `slot_runx<2, 24, false, false>`: the demangled name starts with
    "void whamd::(anonymous namespace)::" -- the bracket of "(anonymous namespace)" is not the argument list's."""
    import argparse
    import bench as b

    pmc = {"_kernel_name": "void whamd::(anonymous namespace)::slot_runx<2, 24, false, false>(whamd::DevProblem, whamd::SlotRun, unsigned int const*, unsigned int*, unsigned int*, unsigned int)",
           "SQ_INSTS_VALU": 1.0e6}
    out = b.roofline_from_counters(pmc, 8.0, "slot_run", 0.0, argparse.Namespace(pmc_variants=8000, coverage=20))
    assert out["kernel"] == "slot_runx<2, 24, false, false>"
    assert out["kernel_filter"] == "slot_run"
