"""Device time of the BOLT #12 text front end (lamd_bolt12_check_text_batch) against the curve work behind it, from lamd_set_timing's HIP events
(lamd_info.last_text_ms), at 64 and at 65 536 strings: the invoices of tests/golden/bolt12_strings.json repeated.  One warm-up call per size, then
three timed calls; the results are compared with the sequential model (tests/bolt12_text_model.py).  DESIGN.md 3.15 quotes it.
Run:  python tools/bolt12_text_bench.py   (needs an MI355X)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bolt12_text_model as M  # noqa: E402
from lightning_amd import Engine  # noqa: E402


def main():
    inv = sorted({r["str"] for r in M.fixture()["strings"] if r["str"].startswith("lni1")})
    want = M.bolt12_check(inv)
    print("%d distinct invoices, mean length %.0f" % (len(inv), sum(map(len, inv)) / len(inv)), flush=True)
    with Engine(0) as eng:
        for n in (64, 65536):
            reps = -(-n // len(inv))
            strings = (inv * reps)[:n]
            for rep in range(4):
                eng.set_timing(rep > 0)
                t = time.time()
                got = eng.bolt12_check(strings)
                wall = (time.time() - t) * 1e3
                ms = eng.info()["last_text_ms"]
                print("n", n, "rep", rep, "wall %.2f ms" % wall, "front end %.3f ms, key parse + curve work + merge %.3f ms, total %.3f ms" %
                      (ms[0], ms[1], ms[0] + ms[1]) if rep else "(warm-up)", flush=True)
            eng.set_timing(False)
            for g, w in zip(got, want):
                assert np.array_equal(g, np.concatenate([w] * reps)[:n])
            assert (got[0] == 0).all()
    print("timing ok")


if __name__ == "__main__":
    main()
