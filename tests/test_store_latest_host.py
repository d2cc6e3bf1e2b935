"""lightning_amd/csrc/store_latest.h on the host, under AddressSanitizer and UBSan (tests/c/store_latest_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the program's own checks of the slot keys, of the 64-bit clock comparisons and of every
new reason on a hand-built store; and the latest-wins repair of the hand-built stores of test_store_latest and of the synthetic store with injected
duplicates, whose reasons, new offsets and output bytes must equal the sequential model of test_store_latest -- in file order, in reverse and in a
scrambled order of the records (the program compares the three itself).  The device side of the same call, lamd_gossip_store_repair_latest, is
test_store_latest's.  Last, the stores the reference ships (test_reference_stores) against the same model."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_store_audit as sa  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_latest as sl  # noqa: E402
from test_store_audit import synthetic  # noqa: E402,F401  (fixture)
from test_store_latest import stores  # noqa: E402,F401  (fixture)

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    sl._entry_refuses_a_null_context()                    # the header the program includes declares what the library exports
    path = str(tmp_path_factory.mktemp("store_latest") / "store_latest_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_latest_host.cpp")])
    return path


def test_keys_clock_rules_and_reasons_under_the_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def _host_repair(exe, d, blob, verdicts, uuid, now, future_slack, prune_interval):
    d.mkdir()
    (d / "image").write_bytes(blob)
    (d / "verdicts").write_bytes(np.array(verdicts, dtype=np.int8).tobytes())
    (d / "uuid").write_bytes(uuid)
    (d / "policy").write_bytes(struct.pack("<QII", now, future_slack, prune_interval))
    r = subprocess.run([exe] + [str(d / x) for x in ("image", "verdicts", "uuid", "policy", "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    return (list((d / "out.reason").read_bytes()), [int(x) for x in np.frombuffer((d / "out.new_off").read_bytes(), dtype="<u8")], (d / "out.image").read_bytes())


CLOCK = dict(now=sl.NOW, future_slack=sl.SLACK, prune_interval=sl.PRUNE)
CASES = [("replay_store", (), sl.OFF), ("replay_store", (), CLOCK), ("bad_record_store", (), sl.OFF),
         ("timestamp_store", (sl.NOW,), dict(CLOCK, prune_interval=0)), ("timestamp_store", (sl.NOW,), sl.OFF), ("timestamp_store", (sl.NOW,), CLOCK),
         ("stale_store", (sl.NOW,), CLOCK), ("stale_store", (sl.NOW,), dict(CLOCK, prune_interval=0)), ("stale_store", (sl.NOW,), sl.OFF),
         ("stale_store", (sl.NOW,), dict(CLOCK, now=sl.NOW + 1)), ("stale_store", (sl.NOW,), dict(CLOCK, now=1000))]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_host_repair_of_the_hand_built_stores_equals_the_model(exe, tmp_path, stores, k):
    name, args, pol = CASES[k]
    built, v = stores.get(name, *args)
    want = sl.latest_model(built[0], v, sl.UUID, **pol)
    assert _host_repair(exe, tmp_path / "r", built[0], v, sl.UUID, **pol) == want
    if (name, pol) in (("replay_store", sl.OFF), ("bad_record_store", sl.OFF), ("stale_store", CLOCK)) or (name == "timestamp_store" and pol == dict(CLOCK, prune_interval=0)):
        assert want[0] == built[1]                        # the reasons the builder lists


def test_host_repair_of_the_store_with_injected_duplicates_equals_the_model(exe, tmp_path, synthetic, stores):
    (blob, added), v = stores.get("injected_store", synthetic[0])
    for k, pol in enumerate((sl.OFF, dict(CLOCK, now=sl.NOW + 3600))):
        want = sl.latest_model(blob, v, sl.UUID, **pol)
        got = _host_repair(exe, tmp_path / str(k), blob, v, sl.UUID, **pol)
        assert got == want and want[0].count(sl.R_SUPERSEDED) >= 1
        # the output repairs to itself: its uuid record is the one record dropped
        n = want[0].count(sl.KEPT) + 1
        again = _host_repair(exe, tmp_path / ("again%d" % k), want[2], [0] * n, sl.UUID, **pol)
        assert again[2] == want[2] and again[0] == [sl.R_BOOKKEEPING] + [sl.KEPT] * (n - 1)


@pytest.mark.parametrize("name", ["part1", "mainnet", "fixed", "canned"])
def test_host_repair_of_the_stores_the_reference_ships_equals_the_model(exe, tmp_path, orc, name):
    """the mainnet excerpt and the canned store of test_reference_stores, without a clock and at their own: the newest header timestamp + 1"""
    blob = rs.store(name)
    v = sa.model(orc, blob)[1]
    for k, pol in enumerate((sl.OFF, dict(CLOCK, now=rs.newest(blob) + 1))):
        want = sl.latest_model(blob, v, sl.UUID, **pol)
        assert _host_repair(exe, tmp_path / str(k), blob, v, sl.UUID, **pol) == want
        assert not {sl.R_SUPERSEDED, sl.R_TIMESTAMP, sl.R_STALE} & set(want[0]) and want[0].count(sl.KEPT) == rs.KEPT[name]
