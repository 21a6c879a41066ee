"""tools/bench_support.py: the statistics, the ordering gate, both sampling schedules and the
result head that every per-call bench tool (tools/<call>_bench.py) takes from it.  The loop's
timer is injected, so the schedules are checked without a device; one GPU test pins that a unit
really is k calls per timed window, from a graph and back to back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import bench_support as B  # noqa: E402

SAMPLES = {"odd": [3.21987, 1.10004, 2.70003, 9.44444, 5.00005],
           "even": [0.51234, 0.49876, 0.50001, 0.53339, 0.47772, 0.52225],
           "ties": [1.0, 1.0, 2.5, 2.5, 2.5, 3.0, 1.0, 3.0]}


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_stats_and_iqr_are_the_numpy_expressions(name):
    xs = SAMPLES[name]
    x = np.array(xs, dtype=np.float64)
    want = {"median": round(float(np.median(x)), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "p25": round(float(np.percentile(x, 25)), 4), "p75": round(float(np.percentile(x, 75)), 4)}
    got = B.stats(xs)
    assert got == want and list(got) == ["median", "min", "max", "p25", "p75"]
    assert B.stats(x) == got  # the tools' two former spellings, with and without dtype=float64, agree
    assert B.iqr(xs) == float(np.percentile(x, 75) - np.percentile(x, 25)) == B.iqr(x)
    assert B.spread(xs) == round(float((np.percentile(x, 75) - np.percentile(x, 25)) / np.median(x)), 4)
    assert xs == SAMPLES[name]  # the samples are not sorted in place


def test_gate_needs_more_than_both_iqrs():
    xs = [1.0, 2.0, 3.0, 4.0, 5.0]  # median 3, IQR 2
    assert B.iqr(xs) == 2.0

    def shifted(d):
        return [x + d for x in xs]  # median 3 + d, IQR 2: the two IQRs sum to 4

    assert B.below_by_more_than_both_iqr(xs, shifted(4.0)) is False  # a difference equal to the sum is not below
    assert B.below_by_more_than_both_iqr(xs, shifted(4.5)) is True
    assert B.below_by_more_than_both_iqr(xs, shifted(3.5)) is False
    assert B.below_by_more_than_both_iqr(shifted(4.5), xs) is False  # it is an ordering, not a distance
    for a in SAMPLES.values():
        for b in SAMPLES.values():
            want = bool(np.median(b) - np.median(a) > B.iqr(a) + B.iqr(b))
            assert B.below_by_more_than_both_iqr(a, b) is want


class ScriptedTimer:
    """Stands in for bench_support.timed: runs `before` and `fn` as it does, so that what they log
    is the order of everything the loop does, and returns 10, 20, 30, ... in turn."""

    def __init__(self):
        self.value = 0.0

    def __call__(self, fn, before=None):
        if before:
            before()
        fn()
        self.value += 10.0
        return self.value


def test_fixed_schedule_keeps_the_order_given_and_drops_the_warmup():
    log = []
    units = {"a": (lambda: log.append("a"), None, 1), "b": (lambda: log.append("b"), lambda: log.append("before_b"), 1),
             "c": (lambda: log.append("c"), None, 1)}
    t = B.sample(units, reps=3, warmup=1, timer=ScriptedTimer())
    assert log == ["a", "before_b", "b", "c"] * 4
    # repetition r times a, b, c as 30 r + 10, + 20, + 30; repetition 0 is the warm-up
    assert t == {"a": [40.0, 70.0, 100.0], "b": [50.0, 80.0, 110.0], "c": [60.0, 90.0, 120.0]}
    assert list(t) == ["a", "b", "c"]


def test_alternating_schedule_reverses_on_odd_repetitions_and_divides_by_k():
    log = []
    ks = {"flows": 2, "a": 2, "a2": 2, "b": 5}
    units = {name: (lambda name=name: log.append(name), None, k) for name, k in ks.items()}
    t = B.sample(units, reps=4, warmup=1, alternate=True, timer=ScriptedTimer())
    up, down = ["a", "a2", "b", "flows"], ["flows", "b", "a2", "a"]
    assert log == up + down + up + down + up  # the index that decides the direction counts the warm-up repetition
    # timer values: rep 0 10..40 (dropped), rep 1 50..80 down, rep 2 90..120 up, rep 3 130..160 down, rep 4 170..200 up
    assert t == {"a": [80 / 2, 90 / 2, 160 / 2, 170 / 2], "a2": [70 / 2, 100 / 2, 150 / 2, 180 / 2],
                 "b": [60 / 5, 110 / 5, 140 / 5, 190 / 5], "flows": [50 / 2, 120 / 2, 130 / 2, 200 / 2]}
    assert list(t) == up


def test_repeated_back_to_back_unit_is_k_calls():
    calls = []
    units = B.repeated({"x": (lambda: calls.append("x"), 3), "y": (lambda: calls.append("y"), 2)}, "back_to_back")
    assert list(units) == ["x", "y"] and [(before, k) for _, before, k in units.values()] == [(None, 3), (None, 2)]
    units["x"][0]()
    units["y"][0]()
    assert calls == ["x"] * 3 + ["y"] * 2


def test_module_imports_without_a_device_and_without_the_library():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", WTP_LIB="/nonexistent/libwtp_crc32.so")
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import bench_support as B; import torch; "
            "assert 'wtp_crc32' not in sys.modules, 'the binding was loaded on import'; "
            "assert not torch.cuda.is_initialized(); print(B.ROOT)")
    out = subprocess.run([sys.executable, "-c", code, TOOLS], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ROOT


def test_common_arguments_and_their_refusals(monkeypatch):
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=50)
    B.add_out(ap, "flows_flush")
    a = ap.parse_args([])
    assert (a.reps, a.warmup, a.inner) == (25, 3, 50)
    assert a.out == os.path.join(ROOT, "profiles", "flows_flush", "flows_flush_bench.json")
    assert list(vars(a)) == ["reps", "warmup", "inner", "out"]
    monkeypatch.setattr(B.torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        B.start("x_bench", a, min_reps=20)
    assert str(e.value) == "x_bench: needs a GPU (no CPU fallback)"
    monkeypatch.setattr(B.torch.cuda, "is_available", lambda: True)
    with pytest.raises(SystemExit) as e:
        B.start("x_bench", ap.parse_args(["--reps", "24"]), min_reps=25)
    assert str(e.value) == "x_bench: --reps must be at least 25"


def test_result_head_comes_first_and_the_file_is_the_printed_line(tmp_path, capsys):
    ap = B.parser()
    B.add_out(ap, "x")
    out = tmp_path / "deeper" / "x_bench.json"  # the directory is made
    a = ap.parse_args(["--reps", "30", "--out", str(out)])
    res = B.result_head("x_bench", a, "a device", "a version", "lib/libwtp_crc32.so")
    assert res == {"tool": "x_bench", "device": "a device", "library": "a version", "lib_path": "lib/libwtp_crc32.so",
                   "reps": 30, "warmup": 3}
    res.update({"goal_ratio": 1.1, "cases": [{"n": 1, "exact": True}]})
    B.write_result(res, a.out)
    printed = capsys.readouterr().out
    assert out.read_text() == printed and printed.endswith("\n") and printed.count("\n") == 1
    back = json.loads(printed)
    assert back == res and list(back) == ["tool", "device", "library", "lib_path", "reps", "warmup", "goal_ratio", "cases"]


@pytest.mark.gpu
def test_every_unit_runs_k_calls_per_timed_window_in_both_modes():
    """Two variants, each an add_(1) on its own counter: x with k = 3, y with k = 2; 1 warm-up and
    2 counted repetitions, alternating.  Back to back the counters end at 3 k; from graphs at
    k more: graph_of's eager run before the capture (the capture itself executes nothing)."""
    import torch
    for how, eager_runs in (("back_to_back", 0), ("graph", 1)):
        cx, cy = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        calls = {"x": (lambda cx=cx: cx.add_(1), 3), "y": (lambda cy=cy: cy.add_(1), 2)}
        t = B.sample(B.repeated(calls, how), reps=2, warmup=1, alternate=True)
        torch.cuda.synchronize()
        assert list(t) == ["x", "y"], how
        for name in t:
            assert len(t[name]) == 2 and all(np.isfinite(ms) and ms > 0 for ms in t[name]), (how, t)
        assert (int(cx.item()), int(cy.item())) == (3 * (3 + eager_runs), 2 * (3 + eager_runs)), how
