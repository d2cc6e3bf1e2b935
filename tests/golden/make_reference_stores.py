#!/usr/bin/env python3
"""The stores and wire vectors the reference ships with expectations of its own authors, as data (tests/test_reference_stores.py,
tests/test_gpu_reference_stores.py, the test_store_*_host.py files):

gossip_store_mainnet_part1.bin, gossip_store_mainnet_part2.bin   contrib/pyln-client/tests/data/gossip_store-part{1,2}.xz unpacked: a mainnet
    excerpt of August 2021; part 2 is a tail to APPEND to part 1 (test_gossmap.py:16-27), not a store of its own.
gossip_store_canned.bin   the bytes of canned_map[] in common/test/run-gossmap_canned.c; common/test/run-gossmap_local.c and
    plugins/renepay/test/run-mcf.c must hold the same bytes.
bolt7_vectors.json   test_vectors_nozlib[] of gossipd/test/run-extended-info.c as parsed JSON, the (update, checksum) pairs of
    connectd/test/run-crc32_of_update.c, the literals run-gossmap_canned.c and pyln's test_gossmap.py assert; every item names its source.

usage: python tests/golden/make_reference_stores.py REFERENCE_TREE"""
import json
import lzma
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _text(ref, rel):
    with open(os.path.join(ref, rel)) as f:
        return f.read()


def _line_of(text, needle):
    return text[:text.index(needle)].count("\n") + 1


def _array(text, name):
    """the bytes of `static u8 NAME[] = { 0x.., ... };`"""
    body = re.search(r"\b%s\[\]\s*=\s*\{(.*?)\};" % name, text, re.S).group(1)
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body))


def _c_strings(text, name):
    """the elements of `static const char *NAME[] = { "..." "...", "...", };`: adjacent literals joined, elements split at the commas between them"""
    body = re.search(r"\*%s\[\]\s*=\s*\{(.*?)\n\};" % name, text, re.S).group(1)
    out, cur = [], None
    for lit, comma in re.findall(r'"((?:[^"\\]|\\.)*)"|(,)', body):
        if comma:
            out.append(cur)
            cur = None
        else:
            cur = (cur or "") + lit.encode().decode("unicode_escape")
    if cur is not None:
        out.append(cur)
    return [s for s in out if s is not None]


def main():
    ref = sys.argv[1]
    sizes = {}

    def write(name, data):
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        sizes[name] = len(data)

    for k in (1, 2):
        with lzma.open(os.path.join(ref, "contrib", "pyln-client", "tests", "data", "gossip_store-part%d.xz" % k), "rb") as f:
            write("gossip_store_mainnet_part%d.bin" % k, f.read())

    canned_c = "common/test/run-gossmap_canned.c"
    ctext = _text(ref, canned_c)
    canned = _array(ctext, "canned_map")
    for rel in ("common/test/run-gossmap_local.c", "plugins/renepay/test/run-mcf.c"):
        assert _array(_text(ref, rel), "canned_map") == canned, rel
    write("gossip_store_canned.bin", canned)

    ext_c = "gossipd/test/run-extended-info.c"
    etext = _text(ref, ext_c)
    vectors = []
    for s in _c_strings(etext, "test_vectors_nozlib"):
        v = json.loads(s)
        v["source"] = "%s:%d" % (ext_c, _line_of(etext, '\\"hex\\" : \\"%s\\"' % v["hex"]))
        vectors.append(v)
    assert [v["msg"]["type"] for v in vectors] == ["QueryChannelRange", "QueryChannelRange", "ReplyChannelRange", "QueryShortChannelIds"]

    crc_c = "connectd/test/run-crc32_of_update.c"
    rtext = _text(ref, crc_c)
    ups = re.findall(r'tal_hexdata\(NULL, "([0-9a-f]+)"', rtext)
    sums = re.findall(r"crc32_of_update\(update\) == (0x[0-9a-f]+)\)", rtext)
    assert len(ups) == len(sums) == 2
    checksums = [dict(update=u, checksum=int(c, 16), source="%s:%d" % (crc_c, _line_of(rtext, "== " + c))) for u, c in zip(ups, sums)]

    ids = re.findall(r'node_id_from_hexstr\("([0-9a-f]{66})"', ctext)
    scid = re.search(r'short_channel_id_from_str\("([0-9x]+)"', ctext).group(1)
    sat = int(re.search(r"AMOUNT_SAT\((\d+)\)", ctext).group(1))
    first = ctext.index("gossmap_chan_get_update_details")
    blocks = [ctext[first:].split("gossmap_chan_get_update_details")[k] for k in (1, 2)]
    dirs = []
    for b in blocks:
        d = {k: int(x) for k, x in re.findall(r"assert\((\w+) == (\d+)\);", b)}
        d.update((k, int(x)) for k, x in re.findall(r"amount_msat_eq\((\w+), AMOUNT_MSAT\((\d+)\)\)", b))
        dirs.append(d)
    assert len(ids) == 2 and [d["channel_flags"] for d in dirs] == [0, 1]
    lo, hi = _line_of(ctext, "node_id_from_hexstr"), _line_of(ctext, "gossmap_chan_get_features") - 2
    canned_lit = dict(node_ids=ids, scid=scid, capacity_sat=sat, directions=dirs, source="%s:%d-%d" % (canned_c, lo, hi))

    py = "contrib/pyln-client/tests/test_gossmap.py"
    ptext = _text(ref, py)
    body = ptext[ptext.index("def test_gossmap("):ptext.index("def test_gossmap_halfchannel(")]
    gone = re.search(r'get_channel\("([0-9x]+)"\) is None', body).group(1)
    gone_node = re.search(r"get_node\('([0-9a-f]{66})'\) is None", body).group(1)
    kept_node = re.search(r"assert g\.get_node\('([0-9a-f]{66})'\)\n", body).group(1)
    chan = re.search(r'channel2 = g\.get_channel\("([0-9x]+)"\)', body).group(1)
    chan_sat = int(re.search(r"channel2\.satoshis == (\d+)", body).group(1))
    lo, hi = _line_of(ptext, 'get_channel("%s") is None' % gone), _line_of(ptext, "channel2.satoshis")
    mainnet_lit = dict(tombstoned_scid=gone, node_pyln_drops=gone_node, node_untouched=kept_node, scid=chan, satoshis=chan_sat,
                       source="%s:%d-%d" % (py, lo, hi))

    doc = dict(extended_queries=vectors, update_checksums=checksums, canned=canned_lit, mainnet=mainnet_lit)
    write("bolt7_vectors.json", (json.dumps(doc, indent=1, sort_keys=True) + "\n").encode())
    for name, n in sizes.items():
        print("%s: %d bytes" % (name, n))


if __name__ == "__main__":
    main()
