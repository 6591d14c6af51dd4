// The parts of the neighbourhood-enrichment kernels (cellenrich.hip) that are plain C++ and run on the host as well -- everything of ITS
// OWN that decides a value, an index or a limit: the permutation generator (fmix, the round keys, the Feistel network F and the
// cycle-walk), the nibble packing of a batch of shuffled classes, the LDS table of the sweep, the flush interval and the limits.  The
// grid, the keys and the pair distance it shares with the other per-slide analyses are in cellgrid_host.h.  Header-only, so a host
// program can exercise them under a sanitizer (tools/dev/cellenrich_host_check.cpp); the kernels and the host-only export
// nuhtc_enrichment_permutation call the same functions.  nuhtc_amd/enrichment.py defines every value (`permutation` is the numpy
// restatement of ce_permute).
//
// The 32-bit budget, stated here once.  The generator is DEFINED mod 2^32: fmix, the key schedule and R + key_k are uint32 and wrap on
// purpose.  A row number is < n <= 2^24 (CE_MAX_POINTS), so n - 1 has at most 24 bits, a half h is at most 12 bits and every value of the
// walk is < 4^h <= 2^24: L, R, x and the shifts by h <= 12 stay far inside 32 bits.  A class nibble is 0 .. C <= 14 < 16.  An LDS table
// entry is uint32: one query has at most n - 1 <= 2^24 - 1 contacts and adds at most that much to any one entry, a block is CE_NT = 256
// queries, and the table is flushed into the int64 outputs at least every ce_flush_blocks(n) blocks, chosen so that
// blocks x 256 x (n - 1) <= 2^32 - 1 (one block at n = 2^24: 256 x (2^24 - 1) = 2^32 - 256).  The outputs are int64: an entry is at most
// n (n - 1) < 2^48.
#pragma once
#include "cellgrid_host.h"

enum { CE_NT = 256, CE_BATCH = 16, CE_ROUNDS = 6, CE_MAX_PERMS = 1024, CE_MAX_CLASSES = CELL_MAX_CLASSES };
constexpr int64_t CE_MAX_POINTS = (int64_t)1 << 24;
constexpr int CE_MAX_CELLS = 1 << 22;                  // one key per cell: at most 2^22 table entries
constexpr int CE_OBS_SLOT = CE_BATCH;                  // the slot of the observed labels in the table of the first sweep
constexpr int CE_MAX_FLUSH_BLOCKS = 64;

// ---- the generator
// the murmur3 finaliser, mod 2^32
CELL_HD inline uint32_t ce_fmix(uint32_t v) {
  v ^= v >> 16; v *= 0x85EBCA6Bu;
  v ^= v >> 13; v *= 0xC2B2AE35u;
  v ^= v >> 16;
  return v;
}

// h, the bits of one half of the Feistel block: max(1, ceil(bitlength(n - 1) / 2)), for n >= 2
CELL_HD inline int ce_half_bits(uint32_t n) {
  int bits = 0;
  for (uint32_t v = n - 1; v; v >>= 1) ++bits;
  const int h = (bits + 1) / 2;
  return h < 1 ? 1 : h;
}

// the six round keys of permutation p (1-based) under `seed`
CELL_HD inline void ce_keys(uint32_t seed, uint32_t p, uint32_t key[CE_ROUNDS]) {
  const uint32_t base = ce_fmix(seed + 0x9E3779B9u * p);
  for (uint32_t k = 0; k < CE_ROUNDS; ++k) key[k] = ce_fmix(base + 0x7F4A7C15u * (k + 1));
}

// F: six rounds of a balanced Feistel network on 2 h bits, a bijection of 0 .. 4^h - 1
CELL_HD inline uint32_t ce_feistel(uint32_t x, int h, const uint32_t key[CE_ROUNDS]) {
  const uint32_t mask = (1u << h) - 1;
  uint32_t L = x >> h, R = x & mask;
#pragma unroll
  for (int k = 0; k < CE_ROUNDS; ++k) {
    const uint32_t t = L ^ (ce_fmix(R + key[k]) & mask);
    L = R; R = t;
  }
  return (L << h) | R;
}

// pi(i) for i < n by cycle-walking: F again while the value is not a row.  F permutes 0 .. 4^h - 1 and i < n lies on a cycle that comes
// back to i < n, so the walk ends; 4^h < 4 n keeps the expected walk under four steps.  n <= 1: the identity.  *steps, when given,
// receives the number of applications of F.
CELL_HD inline uint32_t ce_permute(uint32_t i, uint32_t n, int h, const uint32_t key[CE_ROUNDS], int* steps = nullptr) {
  int s = 0;
  uint32_t x = i;
  if (n > 1)
    do { x = ce_feistel(x, h, key); ++s; } while (x >= n);
  if (steps) *steps = s;
  return x;
}

// ---- the nibble packing: slot s (0 .. 15) of a batch holds a class 0 .. C <= 14 (C: a label outside the classes) in bits 4 s .. 4 s + 3
CELL_HD inline unsigned long long ce_pack(unsigned long long word, int slot, int cls) { return word | ((unsigned long long)(unsigned)cls << (4 * slot)); }
CELL_HD inline int ce_unpack(unsigned long long word, int slot) { return (int)((word >> (4 * slot)) & 15u); }

// ---- the LDS table of one sweep workgroup: uint32 [slots][C + 1][C + 1], slot-major, the row and the column C taking the contacts of a
// label outside the classes (dropped at the flush, so the inner loop has no branch).  The slots 0 .. 15 are the permutations of the
// batch, CE_OBS_SLOT the observed labels (first sweep only).  Within one slot the entries are consecutive words: the lanes of a wave add
// to at most (C + 1)^2 <= 225 of them.
CELL_HD inline int ce_slot_words(int C) { return (C + 1) * (C + 1); }
CELL_HD inline int ce_table_at(int slot, int a, int b, int C) { return slot * ce_slot_words(C) + a * (C + 1) + b; }
constexpr int CE_TABLE_WORDS = (CE_BATCH + 1) * (CE_MAX_CLASSES + 1) * (CE_MAX_CLASSES + 1);     // 3825 words: 15,300 bytes

// how many blocks of CE_NT queries a workgroup may count before it flushes its uint32 table (the budget above)
CELL_HD inline int ce_flush_blocks(int64_t n) {
  if (n <= 1) return CE_MAX_FLUSH_BLOCKS;
  const int64_t k = 0xFFFFFFFFLL / ((int64_t)CE_NT * (n - 1));
  return k < 1 ? 1 : k > CE_MAX_FLUSH_BLOCKS ? CE_MAX_FLUSH_BLOCKS : (int)k;
}

// ---- the front checks of the entry point beside cell_call_ok
inline bool ce_perms_ok(int num_perms) { return num_perms >= 1 && num_perms <= CE_MAX_PERMS; }
inline int ce_batches(int num_perms) { return (num_perms + CE_BATCH - 1) / CE_BATCH; }

// the host-only generator: out[i] = pi_p(i), i < n
inline bool ce_fill_permutation(int64_t n, uint32_t seed, int p, int32_t* out) {
  if (n < 0 || n > CE_MAX_POINTS || p < 1 || p > CE_MAX_PERMS || (n > 0 && !out)) return false;
  uint32_t key[CE_ROUNDS];
  ce_keys(seed, (uint32_t)p, key);
  const int h = n > 1 ? ce_half_bits((uint32_t)n) : 1;
  for (int64_t i = 0; i < n; ++i) out[i] = (int32_t)ce_permute((uint32_t)i, (uint32_t)n, h, key);
  return true;
}
