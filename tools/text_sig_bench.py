"""Device time of the text front ends (lamd_bolt11_check_batch, lamd_checkmessage_batch) against the curve work behind them, from lamd_set_timing's
HIP events (lamd_info.last_text_ms): 100 000 invoices and 100 000 (message, signature) pairs -- 2 000 distinct signed strings each, tiled 50 times --
one warm-up call, then timed calls; the results are compared with the sequential model (tests/text_sig_model.py).  DESIGN.md 3.14 quotes it.
Run:  python tools/text_sig_bench.py   (needs an MI355X)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import text_sig_model as M  # noqa: E402
from lightning_amd import Engine  # noqa: E402

N, DISTINCT = 100000, 2000


def timed(call):
    t = time.time()
    out = call()
    return out, (time.time() - t) * 1e3


def main():
    base = M.random_invoices(DISTINCT, 4242)
    strings = (base * (N // DISTINCT))[:N]
    S = M.Signer(9)
    sec, pub = S.key()
    msgs = [b"message number %d for the timing run" % i for i in range(DISTINCT)]
    zbs = [M.signed_message(S, m, sec, pub) for m in msgs]
    msgs, zbs = (msgs * (N // DISTINCT))[:N], (zbs * (N // DISTINCT))[:N]
    print("mean invoice length", sum(map(len, strings)) / len(strings), flush=True)
    with Engine(0) as eng:
        want = M.bolt11_check(base)
        for rep in range(4):
            if rep == 1:
                eng.set_timing(True)
            got, wall = timed(lambda: eng.bolt11_check(strings))
            info = eng.info()
            print("bolt11 rep", rep, "wall %.2f ms" % wall, "front/curve ms", info["last_text_ms"], "kernel_ms", info["last_kernel_ms"], flush=True)
        for g, w in zip(got, want):
            assert np.array_equal(g, np.concatenate([w] * (N // DISTINCT)))
        print("status histogram", {int(k): int((got[0] == k).sum()) for k in np.unique(got[0])}, "have_n", int(got[3].sum()))
        for rep in range(3):
            mg, wall = timed(lambda: eng.checkmessage(msgs, zbs))
            print("checkmessage rep", rep, "wall %.2f ms" % wall, "front/curve ms", eng.info()["last_text_ms"], flush=True)
        assert (mg[0] == 0).all() and all(bytes(k) == pub for k in mg[1][:50])
    print("timing ok")


if __name__ == "__main__":
    main()
