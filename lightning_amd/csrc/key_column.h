// How many bytes of a caller's key column may be read.  The ABI places key i at pub + i * stride and reads keylen bytes of it, so a column of n
// keys ends with its last KEY, not with the last key's stride: (n - 1) * stride + keylen bytes -- n * stride would run up to stride - keylen bytes
// past a column that is a field at the end of an array of structs.  Every copy of a caller's key column takes its size from here.
// Host code only (no HIP): tests/test_key_column_bytes.py compiles it into a host program.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace lamd {

// *out = (n - 1) * stride + keylen, 0 for n == 0; false (and *out = 0) when that does not fit a size_t or stride < keylen
inline bool key_column_bytes(size_t n, size_t keylen, size_t stride, size_t *out) {
  *out = 0;
  if (n == 0) return true;
  if (stride < keylen) return false;
  const size_t gaps = n - 1;
  if (stride != 0 && gaps > (SIZE_MAX - keylen) / stride) return false;
  *out = gaps * stride + keylen;
  return true;
}

}  // namespace lamd
