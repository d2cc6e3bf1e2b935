#!/usr/bin/env python3
"""tests/golden/query_short_channel_ids_corpus.bin: the reference's fuzz corpus for fromwire_query_short_channel_ids
(tests/fuzz/corpora/fuzz-wire-query_short_channel_ids/, inputs its fuzz target reads), every file prefixed with be16 261 as tests/fuzz/wire.h:15-37
does, packed in the order of the file names: u32 count, then per message u32 length + bytes (little-endian).  The reference's verdicts on
them are recorded nowhere: they are parser inputs on which the header's host build and the model must agree (test_store_query_host.py).
Should the packed file exceed LIMIT bytes, the first files by name that fit are kept; the script prints how many.

usage: python tests/golden/make_query_corpus.py REFERENCE_TREE"""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1 << 20


def main():
    src = os.path.join(sys.argv[1], "tests", "fuzz", "corpora", "fuzz-wire-query_short_channel_ids")
    names = sorted(os.listdir(src))
    body, kept = b"", 0
    for name in names:
        with open(os.path.join(src, name), "rb") as f:
            m = struct.pack(">H", 261) + f.read()
        if 4 + len(body) + 4 + len(m) > LIMIT:
            break
        body += struct.pack("<I", len(m)) + m
        kept += 1
    out = struct.pack("<I", kept) + body
    with open(os.path.join(HERE, "query_short_channel_ids_corpus.bin"), "wb") as f:
        f.write(out)
    print("%d of %d messages, %d bytes" % (kept, len(names), len(out)))


if __name__ == "__main__":
    main()
