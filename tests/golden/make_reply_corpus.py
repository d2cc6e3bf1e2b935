#!/usr/bin/env python3
"""tests/golden/reply_channel_range_corpus.bin: the reference's fuzz corpus for fromwire_reply_channel_range
(tests/fuzz/corpora/fuzz-wire-reply_channel_range/, inputs its fuzz target reads), every file prefixed with be16 264 as tests/fuzz/wire.h:15-37
does, packed in the order of the file names: u32 count, then per message u32 length + bytes (little-endian).  The reference's verdicts on
them are recorded nowhere: they are parser inputs on which the header's host build and the model must agree (test_store_compare_host.py).

usage: python tests/golden/make_reply_corpus.py REFERENCE_TREE"""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    src = os.path.join(sys.argv[1], "tests", "fuzz", "corpora", "fuzz-wire-reply_channel_range")
    names = sorted(os.listdir(src))
    out = struct.pack("<I", len(names))
    for name in names:
        with open(os.path.join(src, name), "rb") as f:
            m = struct.pack(">H", 264) + f.read()
        out += struct.pack("<I", len(m)) + m
    with open(os.path.join(HERE, "reply_channel_range_corpus.bin"), "wb") as f:
        f.write(out)
    print("%d messages, %d bytes" % (len(names), len(out)))


if __name__ == "__main__":
    main()
