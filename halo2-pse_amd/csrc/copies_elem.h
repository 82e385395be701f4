// copies_elem.h -- what copies.hip's kernels do to ONE cell or sort key, host and device: the cell numbering of the ordered permutation
// mapping (include/halo2hip.h, "permutation mapping from copy constraints"), the 64-bit sort key (label << 32) | cell, its order, and
// the successor rule between two neighbouring keys of the sorted, de-duplicated list.  Kept apart from the kernels so that
// tests/cpp/test_copies_host.cpp runs the same source on the host at cell ids no GPU test can afford a mapping for (2^31 and up).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CP_HD __host__ __device__ __forceinline__
#else
#define CP_HD inline
#endif

namespace h2 {

// The key of an endpoint that is not to be sorted in: a copy out of range (device form) and the padding of the last sort tile.  As a
// real key it could only be cell 2^32 - 1 under the label 2^32 - 1: the largest cell as the least of its component, which is then that
// cell alone and maps to itself as the identity fill left it.  The scatter skips the key.
#define CP_PAD_KEY 0xffffffffffffffffull

// id(c, r) = c 2^k + r; the caller has checked c < n_columns, r < 2^k and n_columns 2^k <= 2^32, so the id fits 32 bits
CP_HD uint32_t cp_cell(uint32_t column, uint32_t row, uint32_t k) { return (uint32_t)(((uint64_t)column << k) + row); }
CP_HD uint32_t cp_cell_column(uint32_t cell, uint32_t k) { return (uint32_t)((uint64_t)cell >> k); }
CP_HD uint32_t cp_cell_row(uint32_t cell, uint32_t k) { return (uint32_t)(cell & (((uint64_t)1 << k) - 1)); }

CP_HD uint64_t cp_key(uint32_t label, uint32_t cell) { return ((uint64_t)label << 32) | cell; }
CP_HD uint32_t cp_key_label(uint64_t key) { return (uint32_t)(key >> 32); }
CP_HD uint32_t cp_key_cell(uint64_t key) { return (uint32_t)key; }
// by label, then by cell: unsigned, so that cells 2^31 and up sort above 2^31 - 1
CP_HD bool cp_key_lt(uint64_t a, uint64_t b) { return a < b; }

// `key` is the last of its run of equal keys in the sorted list and `next` the key after it (CP_PAD_KEY at the end of the list): the cell
// that key's cell maps to -- the next cell of the component, or from the component's last cell back to its least one, the label
CP_HD uint32_t cp_successor(uint64_t key, uint64_t next) {
    return next != CP_PAD_KEY && cp_key_label(next) == cp_key_label(key) ? cp_key_cell(next) : cp_key_label(key);
}

}  // namespace h2
