#!/usr/bin/env python3
"""Regenerates tests/golden/text_signatures.json: the STRINGS the reference's own tests hold for its two text-borne signature paths, as data.

  invoices       every "ln..." / "LN..." string literal of common/test/run-bolt11.c, with its line number (the BOLT #11 examples the test
                 decodes, and the ones it asserts a failure for)
  other_strings  the remaining long alphanumeric literals of that file (the example without a separator, :863)
  checkmessage   the (message, zbase, pubkey) triples of tests/test_misc.py (three "contributions from LND users", one of the reference's
                 own), located as tests/golden/make_golden.py locates them

What the reference asserts about them is pinned in tests/test_gpu_text_signatures.py / tests/test_bolt11_host.py, by line number.
Run:  python tests/golden/make_text_signatures.py REFERENCE_TREE   (a Core Lightning checkout; or $LAMD_REFERENCE)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ZCHARS = "ybndrfg8ejkmcpqxot1uwisza345h769"


def harvest(ref):
    out = dict(invoices=[], other_strings=[], checkmessage=[])
    src = os.path.join(ref, "common", "test", "run-bolt11.c")
    for lineno, line in enumerate(open(src, encoding="utf-8", errors="replace"), 1):
        for m in re.finditer(r'"([0-9A-Za-z]{100,})"', line):
            s = m.group(1)
            row = dict(line=lineno, str=s)
            (out["invoices"] if s[:2].lower() == "ln" else out["other_strings"]).append(row)
    zsrc = os.path.join(ref, "tests", "test_misc.py")
    ztxt = open(zsrc, encoding="utf-8").read()
    trip = [(m.start(), m.group(1), m.group(2), m.group(3)) for m in
            re.finditer(r"""\[\s*'@\w+',\s*["']([^"']+)["'],\s*'([%s]{104})',\s*'(0[23][0-9a-f]{64})'\]""" % ZCHARS, ztxt)]
    m2 = re.search(r'msg = "([^"]+)"\s*\n\s*pubkey = "(0[23][0-9a-f]{64})"\s*\n\s*zbase = "([%s]{104})"' % ZCHARS, ztxt)
    if m2:
        trip.append((m2.start(), m2.group(1), m2.group(3), m2.group(2)))
    for pos, msg, zb, pub in trip:
        out["checkmessage"].append(dict(line=ztxt.count("\n", 0, pos) + 1, message=msg, zbase=zb, pubkey=pub))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LAMD_REFERENCE")
    if not ref:
        sys.exit("usage: make_text_signatures.py REFERENCE_TREE")
    out = harvest(ref)
    assert len(out["invoices"]) == 31 and len(out["other_strings"]) == 1 and len(out["checkmessage"]) >= 4, \
        (len(out["invoices"]), len(out["other_strings"]), len(out["checkmessage"]))
    out["source"] = "Core Lightning v26.06.6: common/test/run-bolt11.c, tests/test_misc.py"
    with open(os.path.join(HERE, "text_signatures.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d invoices, %d other, %d checkmessage triples" % (len(out["invoices"]), len(out["other_strings"]), len(out["checkmessage"])))


if __name__ == "__main__":
    main()
