#!/usr/bin/env python3
"""Regenerates tests/golden/bolt12_strings.json: the BOLT #12 STRINGS a Core Lightning checkout holds, as data.

  strings   every "lno1..." / "lnr1..." / "lni1..." (or upper-case) run of at least 20 alphanumeric characters outside tests/fuzz, with file and
            line.  Where the tree's recorded data states an id next to the same string it is kept too: in a JSON document, "offer_id" /
            "local_offer_id" / "invreq_id" of the object that holds the string (doc/schemas/*.json, contrib/msggen/msggen/schema.json); in a
            Python test, 'offer_id' / 'invreq_id' of the literal that the string's statement compares with (tests/test_pay.py)
  recorded  every "offer_id" / "local_offer_id" / "invreq_id": "<64 hex>" those same files state, with file and line: the ids the reference itself
            wrote down.  An invoice answers an invoice request recorded in another document; its invreq_id is found here
  fuzz      a bounded sample of tests/fuzz/corpora/fuzz-bolt12-*-decode: per (kind, status) of the model (tests/bolt12_text_model.py) the
            first 24 files by name of at most 1 200 bytes; bytes as latin-1

What the model says about them is pinned in tests/test_bolt12_text_host.py / tests/test_gpu_bolt12_text.py; the counts are asserted here too.
Run:  python tests/golden/make_bolt12_strings.py REFERENCE_TREE   (or $LAMD_REFERENCE)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bolt12_text_model as M  # noqa: E402

STR = re.compile(rb"(?<![0-9A-Za-z])(?:ln[ior]|LN[IOR])1[0-9A-Za-z]{20,}")
HEX32 = r"([0-9a-f]{64})"
PER_CLASS, MAX_CHARS, MAX_BYTES = 24, 1200, 200 * 1000


def json_ids(doc, found):
    """string -> {offer_id, invreq_id} from the objects that hold both"""
    if isinstance(doc, dict):
        ids = {}
        for key, name in (("offer_id", "offer_id"), ("local_offer_id", "offer_id"), ("invreq_id", "invreq_id")):
            if isinstance(doc.get(key), str) and re.fullmatch(HEX32, doc[key]):
                ids[name] = doc[key]
        if ids:
            for v in doc.values():
                if isinstance(v, str) and STR.fullmatch(v.encode("latin-1", "replace")):
                    for name, hexid in ids.items():
                        assert found.setdefault(v, {}).setdefault(name, hexid) == hexid, (v[:30], name)
        for v in doc.values():
            json_ids(v, found)
    elif isinstance(doc, list):
        for v in doc:
            json_ids(v, found)


IDREC = re.compile(rb"""['"](offer_id|local_offer_id|invreq_id)['"]:\s*['"]([0-9a-f]{64})['"]""")


def harvest(ref):
    rows, recorded = [], []
    for base, dirs, files in os.walk(ref):
        rel = os.path.relpath(base, ref)
        dirs[:] = sorted(d for d in dirs if d != ".git" and os.path.join(rel, d) != os.path.join("tests", "fuzz"))
        for name in sorted(files):
            path = os.path.join(base, name)
            if os.path.islink(path) or not os.path.isfile(path):
                continue
            blob = open(path, "rb").read()
            if b"\0" in blob[:4096] or not STR.search(blob):
                continue
            relpath = os.path.normpath(os.path.join(rel, name))
            lines = blob.split(b"\n")
            ids = {}
            if name.endswith(".json"):
                try:
                    json_ids(json.loads(blob.decode("utf-8")), ids)
                except ValueError:
                    pass
            claimed_until = 0
            for lineno, line in enumerate(lines, 1):
                for m in IDREC.finditer(line):
                    recorded.append(dict(file=relpath, line=lineno, key=m.group(1).decode().replace("local_", ""), hex=m.group(2).decode()))
                for m in STR.finditer(line):
                    s = m.group(0).decode("ascii")
                    row = dict(file=relpath, line=lineno, str=s)
                    row.update(ids.get(s, {}))
                    if name.endswith(".py") and lineno > claimed_until:
                        # the statement the string opens: up to the next blank line.  A string inside it (a payer note) claims nothing
                        end = lineno
                        while end < len(lines) and lines[end].strip():
                            end += 1
                        claimed_until = end
                        text = b"\n".join(lines[lineno - 1:end]).decode("utf-8", "replace")
                        for key in ("offer_id", "invreq_id"):
                            hit = re.search(r"""['"]%s['"]:\s*['"]%s['"]""" % (key, HEX32), text)
                            if hit:
                                row[key] = hit.group(1)
                    rows.append(row)
    return rows, recorded


def fuzz_sample(ref):
    out, seen = [], {}
    root = os.path.join(ref, "tests", "fuzz", "corpora")
    for corpus in sorted(os.listdir(root)):
        if not re.fullmatch(r"fuzz-bolt12-.*-decode", corpus):
            continue
        for name in sorted(os.listdir(os.path.join(root, corpus))):
            blob = open(os.path.join(root, corpus, name), "rb").read()
            if len(blob) > MAX_CHARS:
                continue
            f = M.bolt12_front(blob)
            cls = (f["kind"], f["status"])
            if seen.get(cls, 0) >= PER_CLASS:
                continue
            seen[cls] = seen.get(cls, 0) + 1
            out.append(dict(corpus=corpus, name=name, str=blob.decode("latin-1")))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LAMD_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    strings, recorded = harvest(ref)
    fx = dict(strings=strings, recorded=recorded, fuzz=fuzz_sample(ref))
    p = M.pinned(fx, M.bolt12_check)
    print(p)
    assert p["ok_invoices"] == 7 and p["ok_invreqs"] == 2 and p["ok_offers"] == 7, p
    assert p["no_key_invreqs"] == [os.path.join("tests", "test_pay.py")], p
    assert p["offers_with_offer_id"] >= 3 and p["invoices_with_offer_id"] >= 3, p
    assert p["invreqs_with_invreq_id"] >= 2 and p["invoices_with_invreq_id"] >= 1, p
    text = json.dumps(fx, indent=0, sort_keys=True) + "\n"
    assert len(text) < MAX_BYTES, len(text)
    open(os.path.join(HERE, "bolt12_strings.json"), "w").write(text)
    print("%d strings, %d recorded ids, %d fuzz inputs, %d bytes" % (len(fx["strings"]), len(fx["recorded"]), len(fx["fuzz"]), len(text)))


if __name__ == "__main__":
    main()
