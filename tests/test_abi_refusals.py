"""The protocol entry points' answers before any device is touched (return code and
wtp_last_error() for every documented violation and every ordered pair of them, the no-op
shapes, and every *_work_bytes value over a grid) equal tests/golden/abi_refusals.json, which
tests/golden/make_abi_refusals.py recorded: which message two bad arguments give, and what a
work buffer must hold, are part of the C-ABI, whatever the host code behind them looks like.
No case reaches a launch, so no GPU is needed."""
import json
import os
import types

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    # compiled here, not imported: an import would leave a bytecode cache under tests/golden/
    path = os.path.join(GOLDEN, "make_abi_refusals.py")
    mod = types.ModuleType("make_abi_refusals")
    mod.__file__ = path
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), mod.__dict__)
    return mod


@pytest.fixture(scope="module")
def got(gen):
    import wtp_crc32 as W
    return gen.cases(W.LIB)


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "abi_refusals.json")) as f:
        return json.load(f)


def test_every_protocol_call_is_covered(want):
    import wtp_crc32 as W
    assert len(want["refusals"]) == 15 and set(want["refusals"]) <= set(W.EXPORTED)
    assert set(want["work_bytes"]) == {n for n in W.EXPORTED if n.endswith("_work_bytes")}
    for call, rows in want["refusals"].items():
        singles = [k for k in rows if " + " not in k and not k.startswith("ok: ")]
        assert len(singles) >= 4 and any(" + " in k for k in rows), call
        for k, (rc, msg) in rows.items():
            assert (rc, msg) == (0, "") if k.startswith("ok: ") else (rc == -1 and msg), (call, k)


def test_refusals_and_messages(got, want):
    assert list(got["refusals"]) == list(want["refusals"])
    for call, rows in want["refusals"].items():
        assert list(got["refusals"][call]) == list(rows), call
        diff = {k: (got["refusals"][call][k], v) for k, v in rows.items() if got["refusals"][call][k] != v}
        assert not diff, (call, diff)


def test_work_bytes(got, want):
    assert got["work_bytes"] == want["work_bytes"]


def test_file_is_what_the_generator_writes(gen, got):
    with open(os.path.join(GOLDEN, "abi_refusals.json")) as f:
        assert f.read() == gen.render(got)
