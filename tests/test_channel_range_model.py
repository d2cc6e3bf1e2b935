"""What the tests of the channel digest and of the query_channel_range answers stand on (channel_range_model.py), and the boundary of the new calls:
the model's CRC-32C against the RFC 3720 check value and the header CRCs of the stores the reference's gossipd wrote; the four uncapped reply limits;
on both golden stores the sorted answer against the answer in the reference's own order -- equal as multisets, and for the mesh store NOT in the same
order, which is the one deliberate difference from the reference; and that include/lightning_amd.h declares the new calls and the library exports them."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402

GOLDEN = ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin")
NEW = ("lamd_gossip_store_digest_build", "lamd_store_digest_free", "lamd_store_digest_count", "lamd_store_digest_read", "lamd_channel_range_reply_batch")


def test_crc32c_is_rfc_3720s_and_the_reference_stores_own():
    assert sa.crc32c(0, b"123456789") == 0xE3069283
    assert sa.crc32c(0, bytes(32)) == 0x8A9136AA and sa.crc32c(0, b"\xff" * 32) == 0x62A8AB43      # RFC 3720 B.4
    for name in GOLDEN:
        recs = sa.walk(sa._golden(name))[0]
        assert len(recs) >= 6
        for _, _, crc, ts, m in recs:
            assert sa.crc32c(ts, m) == crc
    # seeding with the first part's CRC is the CRC of the two parts joined: how crc32_of_update chains them
    m = bytes(range(200))
    assert crm.update_csum(m) == sa.crc32c(0, m[66:106] + m[110:])


def test_the_four_uncapped_limits_and_capped_ones():
    assert [crm.limit(o) for o in range(4)] == [8186, 4092, 4092, 2728]
    assert [crm.limit(0, c) for c in (1, 8, 15, 16, 24, 56, 63, 1 << 30)] == [1, 1, 1, 2, 3, 7, 7, 8186]
    assert [crm.limit(3, c) for c in (1, 24, 47, 48, 168)] == [1, 1, 1, 2, 7]
    for o in range(4):                                    # a full reply fits a message, one entry more does not
        e = [(k, (1, 2), (3, 4), (0, 0, 0)) for k in range(crm.limit(o) + 1)]
        assert len(crm.encode(crm.CHAIN, 0, 1, e[:-1], 1, o)) <= 65535 < len(crm.encode(crm.CHAIN, 0, 1, e, 1, o))


@pytest.mark.parametrize("name", GOLDEN)
def test_sorted_answer_holds_what_the_reference_order_holds(name):
    blob = sa._golden(name)
    ref, counters = crm.digest(blob)
    ours = crm.sorted_digest(blob)[0]
    key = lambda e: e[:3]
    assert sorted(map(key, ours)) == sorted(map(key, ref)) and len(ours) == counters["entries"] == counters["channels"] > 0
    assert [e[0] for e in ours] == sorted(e[0] for e in ours)
    blocks = [e[0] >> 40 for e in ref]
    for first, number in ((0, 0xFFFFFFFF), (min(blocks), 1), (min(blocks) + 1, max(blocks) - min(blocks) - 1), (max(blocks), 5), (0, min(blocks))):
        number = crm.fix_number(first, number)
        a, b = crm.gather_range(ref, first, number), crm.gather_range(ours, first, number)
        assert sorted(map(key, a)) == sorted(map(key, b))
        assert b == sorted(b)
    if name == "gossip_store_mesh_3x3.bin":
        assert len(ref) == 12 and [e[0] for e in ref] != sorted(e[0] for e in ref)          # the reference's order is not BOLT #7's
        assert blocks[:7] == [103, 105, 107, 109, 113, 115, 111]
    # every update the model checksums is one the reference wrote: 40 + (len - 110) bytes go in
    for e in ours:
        for d in (0, 1):
            if e[3][1 + d] != crm.NONE:
                m = sa.walk(blob)[0][e[3][1 + d]][4]
                assert m[:2] == b"\x01\x02" and (m[111] & 1) == d and int.from_bytes(m[98:106], "big") == e[0] and int.from_bytes(m[106:110], "big") == e[1][d]


def test_split_properties_of_the_model():
    """the properties the device test asserts of every answer, on the model itself: entries in order, blocks summing to the request, first_blocknums
    chaining, the last reply alone complete"""
    store = crm.population_store([1, 2, 3, 4, 10])
    e = crm.sorted_digest(store)[0]
    assert len(e) == 20
    for cap in (0, 8, 16, 24, 56):
        for q in crm.query_kinds([100, 103, 106, 109, 112]):
            st, rs = crm.replies(e, crm.CHAIN, q, cap)
            if st != 0:
                assert len(rs) == (1 if st == 1 else 0)
                continue
            _, first, number, _ = crm.parse_query(q)
            number = crm.fix_number(first, number)
            ds = [crm.decode_reply(r) for r in rs]
            assert [s for d in ds for s in d["scids"]] == [x[0] for x in crm.gather_range(e, first, number)]
            assert sum(d["blocks"] for d in ds) == number and ds[0]["first"] == first
            assert all(a["first"] + a["blocks"] == b["first"] for a, b in zip(ds, ds[1:]))
            assert [d["final"] for d in ds] == [0] * (len(ds) - 1) + [1]


def test_new_calls_are_declared_exported_and_refuse_null(tmp_path):
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(sa.ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    lib = _ffi.load()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in _ffi.SYMBOLS, n
    assert lib.lamd_store_digest_count(None) == 0 and lib.lamd_store_digest_read(None, 0, None, None, None, None) == -3
    lib.lamd_store_digest_free(None)
    s, r = _ffi.LamdStoreDigestSummary(), _ffi.LamdRangeReplySummary()
    assert lib.lamd_gossip_store_digest_build(None, None, 0, None, 0, None, None, None, ctypes.byref(s)) == -3
    assert lib.lamd_channel_range_reply_batch(None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, ctypes.byref(r)) == -3
    # the ctypes mirrors of the two summaries are laid out as the header's
    for cname, cls in (("lamd_store_digest_summary", _ffi.LamdStoreDigestSummary), ("lamd_range_reply_summary", _ffi.LamdRangeReplySummary)):
        fields = [f[0] for f in cls._fields_]
        src = tmp_path / (cname + ".c")
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n  printf("%%zu\\n", sizeof(%s));\n' % cname
                       + "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "  return 0;\n}\n")
        exe = tmp_path / cname
        subprocess.check_call(["gcc", "-I" + os.path.join(sa.ROOT, "include"), "-o", str(exe), str(src)])
        out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
        assert out[0] == ctypes.sizeof(cls) and out[1:] == [getattr(cls, f).offset for f in fields]
        body = re.search(r"typedef struct[^{;]*\{([^}]*)\} %s;" % cname, hdr, re.S).group(1)
        assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[[^\]]*\])?\s*[,;]", body) == fields
