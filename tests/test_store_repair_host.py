"""lightning_amd/csrc/store_repair.h on the host, under AddressSanitizer and UBSan (tests/c/store_repair_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the program's own checks of the node table, of the copy at every source and output
alignment and of every keep rule on a hand-built store; and the repair of the synthetic store of test_store_audit and of its damaged copy,
whose keep flags, reasons, new offsets and output bytes must equal the Python model of test_store_repair (verdicts by test_store_audit.model);
and the same for the stores the reference ships (test_reference_stores)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_store_audit as sa  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_repair as sr  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_repair") / "store_repair_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_repair_host.cpp")])
    return path


def test_node_table_copy_and_keep_rules_under_the_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def _host_repair(exe, tmp_path, blob, verdicts, uuid):
    (tmp_path / "image").write_bytes(blob)
    (tmp_path / "verdicts").write_bytes(np.array(verdicts, dtype=np.int8).tobytes())
    (tmp_path / "uuid").write_bytes(uuid)
    r = subprocess.run([exe, str(tmp_path / "image"), str(tmp_path / "verdicts"), str(tmp_path / "uuid"), str(tmp_path / "out")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    return (list((tmp_path / "out.reason").read_bytes()), [int(x) for x in np.frombuffer((tmp_path / "out.new_off").read_bytes(), dtype="<u8")],
            (tmp_path / "out.image").read_bytes())


def test_host_repair_of_the_synthetic_and_the_damaged_store_equals_the_model(exe, tmp_path, orc, synthetic, damaged):
    img, (_, sv, _) = synthetic
    blob, (_, dv, _), classes = damaged
    for k, (image, verdicts) in enumerate(((img, sv), (blob, dv))):
        d = tmp_path / str(k)
        d.mkdir()
        want = sr.repair_model(image, verdicts, sr.UUID)
        reason, new_off, out = _host_repair(exe, d, image, verdicts, sr.UUID)
        assert reason == want[0]                          # the reasons, and with them the keep flags
        assert [x == sr.KEPT for x in reason] == [x != sr.DROPPED for x in new_off]
        assert new_off == want[1] and out == want[2]
        assert len(out) <= len(image) + 46 and 0 < want[0].count(sr.KEPT) < len(reason)
    # the damaged store shows every reason, and each class of damage the one it must
    expect = {"body": sr.R_VERDICT, "sig": sr.R_VERDICT, "direction": sr.R_VERDICT, "orphan": sr.R_DEPENDENCY, "moved": sr.R_DEPENDENCY, "copy": sr.R_VERDICT,
              "unknown": sr.R_VERDICT, "truncated": sr.R_VERDICT}
    assert set(reason) == {0, 1, 2, 3, 4}
    for i, c in enumerate(classes):
        assert c is None or reason[i] == expect[c], (i, c, reason[i])


def test_host_repair_of_the_reference_stores_equals_compactd(exe, tmp_path, orc):
    for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"):
        d = tmp_path / name
        d.mkdir()
        blob = sa._golden(name)
        assert _host_repair(exe, d, blob, sa.model(orc, blob)[1], sr.UUID)[2] == sr.compactd_first_phase(blob, sr.UUID)


@pytest.mark.parametrize("name", ["part1", "mainnet", "fixed", "canned"])
def test_host_repair_of_the_stores_the_reference_ships_equals_the_model(exe, tmp_path, orc, name):
    """the mainnet excerpt (its first part, both parts, both with the tombstone's CRC corrected) and the canned store of test_reference_stores"""
    blob = rs.store(name)
    verdicts = sa.model(orc, blob)[1]
    want = sr.repair_model(blob, verdicts, sr.UUID)
    assert _host_repair(exe, tmp_path, blob, verdicts, sr.UUID) == want
    if name in ("part1", "canned"):
        assert want[2] == sr.compactd_first_phase(blob, sr.UUID)
    else:                                                 # the last announcement has the tombstone behind it, not an amount record
        assert want[0][-2:] == [sr.R_DEPENDENCY, sr.R_VERDICT if name == "mainnet" else sr.R_BOOKKEEPING] and want[0].count(sr.KEPT) == rs.KEPT[name]
