#!/usr/bin/env python3
"""node_announcements.json: the distinct node_announcement literals of the reference's lightningd/test/run-check_node_announcement.c, copied as
data (tests/test_store_nodes_host.py receives them): one plain, one with an all-zero signature, one with an option_will_fund TLV.  Each carries
the status lamd_node_announcement_receive_batch must give it against an EMPTY directory (nothing pending), decided by the sequential model of
tests/node_receive_model.py with the C oracle's sigcheck_node_announcement for the signature -- nobody here authored these inputs.

usage: python tests/golden/make_node_announcements.py REFERENCE_TREE"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "lightningd/test/run-check_node_announcement.c"


def main():
    ref = sys.argv[1]
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import node_receive_model as nrm
    from oracle import orc
    with open(os.path.join(ref, SOURCE)) as f:
        text = f.read()
    items, seen = [], set()
    for k, line in enumerate(text.split("\n"), 1):
        for lit in re.findall(r'tal_hexdata\([^,]*,\s*"([0-9a-fA-F]+)"', line):
            if lit.lower() in seen:
                continue
            seen.add(lit.lower())
            m = bytes.fromhex(lit)
            parsed = nrm.parse(m)
            status = nrm.receive(nrm.view(b"\x10"), [m], nrm.checker(orc))["status"][0]
            f_len = int.from_bytes(m[66:68], "big")
            end = 68 + f_len + 4 + 70 + int.from_bytes(m[68 + f_len + 4 + 68:68 + f_len + 4 + 70], "big")
            items.append(dict(source="%s:%d" % (SOURCE, k), hex=lit.lower(), status=status, zero_signature=m[2:66] == bytes(64), tlv_bytes=len(m) - end,
                              oracle_sigcheck=orc.sigcheck_node_announcement(m), timestamp=None if parsed is None else parsed[0]))
    with open(os.path.join(HERE, "node_announcements.json"), "w") as f:
        json.dump(dict(source=SOURCE, announcements=items), f, indent=1)
        f.write("\n")
    print("%d announcements: statuses %s" % (len(items), [i["status"] for i in items]))


if __name__ == "__main__":
    main()
