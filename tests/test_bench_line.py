"""The driver reads bench.py's result out of an 8 KB tail of stdout (BENCH_r04.json came back ``parsed: null`` for a 30.6 KB line):
the ONE stdout line must stay a compact object that round-trips through json.loads and keeps the contract's keys."""
import glob
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


FULL = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_bench_default.json")))


@pytest.mark.parametrize("path", FULL[-3:], ids=os.path.basename)
def test_compact_line_fits_the_driver_tail(path):
    b = _bench()
    full = json.load(open(path))
    full["_precision"] = "bf16"
    line = json.dumps(b.compact(full))
    assert len(line) < b.COMPACT_LIMIT <= 8192, len(line)
    back = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config"):
        assert k in back, k
    assert back["value"] == full["value"] and back["config"]["workload"] == full["config"]["workload"]
    if "roofline" in full:
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in back["roofline"], k
    if "cpu_baseline" in full:
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in back["cpu_baseline"], k


def test_compact_line_survives_a_bloated_record():
    """whatever later rounds add to the full record, the line sheds optional blocks instead of growing"""
    b = _bench()
    full = json.load(open(FULL[-1]))
    full["_precision"] = "bf16"
    full["configs"].update({f"extra {i}": dict(full["configs"]["configs[2]"]) for i in range(40)})
    line = json.dumps(b.compact(full))
    assert len(line) < b.COMPACT_LIMIT
    back = json.loads(line)
    assert "roofline" in back and "cpu_baseline" in back and back["value"] == full["value"]


def test_plain_line_keeps_the_contract_without_profile_fields():
    """a run without --full measures no profiled block: its line keeps the contract's keys and names no committed profiles"""
    b = _bench()
    full = json.load(open(FULL[-1]))
    plain = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                  "vs_baseline", "dtype", "data", "config", "rtf", "ms_per_euler_step", "hip_event_median_ms")}
    assert not b.has_profiled_blocks(plain) and b.has_profiled_blocks(full)
    back = json.loads(json.dumps(b.compact(plain)))
    assert {k: back[k] for k in plain} == plain
    assert "profiles_head" not in back and "abs_err_measured" not in back


def test_dump_outputs_stays_in_budget_and_samples_the_same_rows(tmp_path):
    """--dump-outputs: float32 files; a batch over the budget is cut to the same seeded rows on every run, their indices stored beside it"""
    import numpy as np
    b = _bench()
    b.DUMP_LIMIT = 1 << 20
    small = np.arange(2 * 80 * 16, dtype=np.float64).reshape(2, 80, 16)
    assert b.dump_outputs(str(tmp_path / "s"), {"mel": small}) == {"mel": [2, 80, 16]}
    got = np.load(tmp_path / "s" / "mel.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.astype(np.float32))
    big = np.random.default_rng(3).standard_normal((64, 80, 256)).astype(np.float32)       # 5.2 MB
    shapes = [b.dump_outputs(str(tmp_path / d), {"mel": big}) for d in ("a", "b")]
    assert shapes[0] == shapes[1] and shapes[0]["mel"][0] < 64
    for d in ("a", "b"):
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= b.DUMP_LIMIT
    rows = np.load(tmp_path / "a" / "mel_rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "mel_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "mel.npy"), big[rows.astype(np.int64)])


def test_bench_has_no_unresolved_global_names():
    """bench.py's GPU-only branches never run in the CPU suite: a name that resolves nowhere (round 6: `np` in job_abs_err) would only
    surface in the driver's run.  Every implicitly-global name referenced inside any function of bench.py must be defined at module
    level or be a builtin."""
    import builtins
    import os
    import symtable
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    top = symtable.symtable(src, "bench.py", "exec")
    defined = {s.get_name() for s in top.get_symbols() if s.is_assigned() or s.is_imported() or s.is_namespace()} | set(dir(builtins))
    missing = []

    def walk(tab):
        for ch in tab.get_children():
            for s in ch.get_symbols():
                if s.is_referenced() and s.is_global() and s.get_name() not in defined:
                    missing.append((ch.get_name(), s.get_name()))
            walk(ch)

    walk(top)
    assert not missing, missing
