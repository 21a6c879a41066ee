"""The two-slab pipeline driver of the host-memory calls (csrc/wtp_slab_pipe.hpp) needs no
GPU: tests/slab_pipe_check.cpp drives wtp::run_slabs with recording callbacks, built with
the address and undefined-behaviour sanitizers and run as a child process.  The expected
orders are those of the hand-written loops the driver replaced (wtp_host.cpp before it):
slab s on buffer s % 2, a buffer's previous slab retired just before it is issued again,
the last two slabs retired at the end."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a3-reliable-transport_amd", "csrc")

# (n, per) -> calls in order: I/R <buffer>[<first>+<count>]
EXPECTED = {
    (0, 1): "",
    (0, 2): "",
    (0, 7): "",
    (1, 1): "I0[0+1] R0[0+1]",
    (1, 2): "I0[0+1] R0[0+1]",
    (1, 7): "I0[0+1] R0[0+1]",
    (2, 1): "I0[0+1] I1[1+1] R0[0+1] R1[1+1]",
    (2, 2): "I0[0+2] R0[0+2]",
    (2, 7): "I0[0+2] R0[0+2]",
    (3, 1): "I0[0+1] I1[1+1] R0[0+1] I0[2+1] R1[1+1] R0[2+1]",
    (3, 2): "I0[0+2] I1[2+1] R0[0+2] R1[2+1]",
    (3, 7): "I0[0+3] R0[0+3]",
    (5, 1): "I0[0+1] I1[1+1] R0[0+1] I0[2+1] R1[1+1] I1[3+1] R0[2+1] I0[4+1] R1[3+1] R0[4+1]",
    (5, 2): "I0[0+2] I1[2+2] R0[0+2] I0[4+1] R1[2+2] R0[4+1]",
    (5, 7): "I0[0+5] R0[0+5]",
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slab_pipe") / "slab_pipe_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wshadow", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "slab_pipe_check.cpp"),
                    "-o", exe], check=True)

    def run(*cases):
        """[(n, per, fail_issue, fail_retire), ...] -> [(calls, rc), ...], one child process."""
        p = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        lines = p.stdout.splitlines()
        assert len(lines) == len(cases)
        return [(l.rsplit("|rc=", 1)[0], int(l.rsplit("|rc=", 1)[1])) for l in lines]
    return run


def _calls(text):
    return [(w, int(b), int(f), int(c)) for w, b, f, c in re.findall(r"([IR])(\d)\[(\d+)\+(\d+)\]", text)]


def test_order_of_calls_is_the_replaced_loops(check):
    keys = sorted(EXPECTED)
    assert keys == [(n, per) for n in (0, 1, 2, 3, 5) for per in (1, 2, 7)]
    got = check(*[(n, per, 0, 0) for n, per in keys])
    assert got == [(EXPECTED[k], 0) for k in keys]


def test_every_item_once_and_no_buffer_issued_while_live(check):
    cases = [(n, per, 0, 0) for n in range(0, 20) for per in (1, 2, 3, 7, 19, 64)]
    for (n, per, _, _), (text, rc) in zip(cases, check(*cases)):
        calls = _calls(text)
        assert rc == 0 and len(text.split()) == len(calls)
        nxt, live, slab = 0, {}, 0
        for what, b, first, count in calls:
            if what == "I":
                assert b == slab % 2 and b not in live, (n, per, text)
                assert first == nxt and count == min(per, n - first) and count > 0, (n, per, text)
                live[b] = (first, count)
                nxt += count
                slab += 1
            else:  # retires what was issued on that buffer, once
                assert live.pop(b, None) == (first, count), (n, per, text)
            assert len(live) <= 2
        assert nxt == n and not live, (n, per, text)
        assert slab == -(-n // per)


def test_a_failing_call_stops_the_pipeline_at_once(check):
    third_issue, second_retire, last_retire, first_issue = check((5, 1, 3, 0), (5, 1, 0, 2), (5, 2, 0, 3), (5, 2, 1, 0))
    # slabs 0 and 1 issued, slab 0 retired, slab 2's issue fails: slab 1 stays live for the caller's drain
    assert third_issue == ("I0[0+1] I1[1+1] R0[0+1] I0[2+1]", 7)
    assert second_retire == ("I0[0+1] I1[1+1] R0[0+1] I0[2+1] R1[1+1]", 9)
    assert last_retire == (EXPECTED[(5, 2)], 9)
    assert first_issue == ("I0[0+2]", 7)


def test_a_slab_size_of_zero_calls_nothing(check):
    assert check((5, 0, 0, 0), (0, 0, 0, 0)) == [("", -1), ("", 0)]
