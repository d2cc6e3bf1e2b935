"""The strict reader of a verdict column the library wrote.  include/lightning_amd.h promises that every such byte is 0 or 1; the kernels' own
markers (2: BIP-340 parity / recovery pending, 3: suspect) and a test's pre-fill (9) all compare equal to True under .astype(bool), so the tests
read raw verdict bytes through strict_bool() instead."""
import numpy as np


def strict_bool(raw_uint8):
    """raw uint8 verdicts (numpy, or anything np.asarray takes) -> bool array; asserts that every byte is 0 or 1"""
    raw = np.asarray(raw_uint8)
    assert raw.dtype == np.uint8, raw.dtype
    bad = np.flatnonzero(raw.reshape(-1) > 1)
    assert not bad.size, "%d of %d verdict bytes are neither 0 nor 1; first (row, byte): %s" % (
        bad.size, raw.size, [(int(i), int(raw.reshape(-1)[i])) for i in bad[:8]])
    return raw.astype(bool)
