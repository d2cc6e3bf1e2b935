"""Run by tests/test_gpu_tables.py in a process of its own, where no other engine keeps the device's G table alive (in a whole-suite run the pytest
process holds engines of its own, e.g. the one behind liblightning_amd_cln.so): here the first engine BUILDS the table and, after every engine
is closed, the next one builds it again.  Prints one JSON line: the two creation times, the time and the result of a full audit after each build's
warm-up call, and the audits of one full window and of the window-boundary slices of the rebuilt table."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BITS, NWIN = 24, 11
ENTRIES = NWIN << BITS


def main():
    import torch
    from lightning_amd import Engine
    out = {}
    free0 = torch.cuda.mem_get_info(0)[0]
    t0 = time.perf_counter()
    e = Engine(0)
    out["t_create"] = time.perf_counter() - t0
    out["table_allocated_by_create"] = free0 - torch.cuda.mem_get_info(0)[0] >= ENTRIES * 64
    e.gtable_audit(0, 256)                      # the audit kernel's code is loaded before the clock starts
    t0 = time.perf_counter()
    out["full"] = e.gtable_audit(0, ENTRIES)
    out["t_audit"] = time.perf_counter() - t0
    e.close()
    free1 = torch.cuda.mem_get_info(0)[0]
    t0 = time.perf_counter()
    e = Engine(0)
    out["t_create_again"] = time.perf_counter() - t0
    out["table_allocated_again"] = free1 - torch.cuda.mem_get_info(0)[0] >= ENTRIES * 64
    out["window7"] = e.gtable_audit(7 << BITS, 1 << BITS)
    out["slices"] = [e.gtable_audit(0, 257)] + [e.gtable_audit((w << BITS) - 3, 7) for w in range(1, NWIN)] + [e.gtable_audit(ENTRIES - 3, 3)]
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
