// The EXPECTO_* tuning knobs of a Beluga handle (INTEGRATION.md lists them): their fields with the
// defaults, and the one table that reads them from the environment.  Host only (no HIP include),
// so tests/beluga_knobs_driver.cpp builds it with the host compiler alone.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <limits>

namespace expecto {

// FC1 split-K: a fixed number of slabs per handle (default 8 of 8480; a divisor of
// 67840/32 = 2120 K blocks), whatever the batch, so an FC1 output never depends on how many
// windows shared the launch.
constexpr int kFc1KBlocks = 2120;
constexpr int kFc2KBlocks = 63;
constexpr int kFc2SplitsDefault = 7;   // FC2 K = 63 blocks of 32 -> 7 slabs of 9: a 2000-row FC2 fills
                                        // 728 workgroups instead of 104 (fixed: sums never depend on M)
constexpr int kFcSplitsDefault = 8;    // round 2 sweep (tools/knob_sweep.py, interleaved): 8 vs 20 slabs
                                       // +0.6-0.9 % on the 200-window workload, +0.3-1.2 % on configs[1]
                                       // (4: -0.6 / -3.7 %), with 2.5x less split-K partial traffic

// Default Karatsuba FC1 slice of the segment path, in max_batch windows: the 200-window workload's
// chunk (both strands of 96 SNVs, 38,400 windows at max_batch 8192: 4.69 max_batch) is one slice; a
// larger chunk runs in slices.  The slice's buffers (beluga.hip fk_seg_buffers) are sized by it.
constexpr int kFkSlicePerBatch = 5;

struct BelugaKnobs {
  bool overlap = true;                //   EXPECTO_OVERLAP=0: one stream (same bits either way)
  int fc_splits = kFcSplitsDefault;   // FC1 split-K slabs: a divisor of 2120 K blocks, <= 32
  int fc2_splits = kFc2SplitsDefault; // FC2 split-K slabs: a divisor of 63 K blocks
  int fc2_rows_env = 0;               // EXPECTO_FC2_ROWS as given (>= 1; 0: unset); create derives fc2_rows from it
  double fc1_m_order_mb = 80.0;       // FC1 dispatch: M tiles fastest while one split's A is <= this
  int fc1_order = 3;                  // FC1 dispatch order (EXPECTO_FC1_ORDER): 3 grouped M tiles (default),
                                      // 0 M-fastest / N-fastest by A-slab size, 2 slab-outermost
  int fc1_m_group = 8;                // order 3: M tiles per group (EXPECTO_FC1_M_GROUP)
  bool fc_wide = true;                // f16x3 FC split-K GEMMs on 336-column tiles (EXPECTO_FC_WIDE; same bits)
  int conv_tile = 0;                  // f16x3 conv M tile: 0 = auto (conv_tile_rows), 256 or 384
  bool conv_ea = true;                // f16x3 conv consumers' early next-stage reads (EXPECTO_CONV_EA)
  bool fc_skinny = true;              // FC1 / FC2 of <= 32 rows on 32 x 32 tiles (EXPECTO_FC_SKINNY; same bits)
  int fc1_narrow = -1;                // grouped FC1 tile width: -1 auto (fc1_narrow), 0 336, 1 112 columns
  int conv_narrow = -1;               // conv5 / conv6 tile width: -1 auto (conv_narrow), 0 160, 1 64 columns
  int seg_chunk_windows = 0;          // segment path: windows per chunk cap (0 = none; tuning knob)
  bool seg_merge_strands = true;      // segment path: a chunk may hold entries of both strands (EXPECTO_SEG_MERGE_STRANDS)
  bool pool_one_pass = true;          // segment path: pool2 of all phases in one pass (same bits)
  bool pool_fused = true;             // segment path, phases {0, 2}: pool2 in conv4's epilogue (EXPECTO_POOL_FUSED; same bits)
  bool fuse_conv1 = true;             // f16x3 codes input: conv1 inside the conv2 launch (EXPECTO_FUSE_CONV1; same bits)
  bool kmer_on = true;                // f16x3 codes input: conv1 + conv2 + pool1 from the k-mer table (EXPECTO_CONV2_TABLE)
  bool kmer_quad = true;              //   conv2 rows from the quad tables (EXPECTO_KMER_QUAD=0: pair tables only)
  double kmer_max_bytes = std::numeric_limits<double>::infinity();   //   cap on the table's bytes (EXPECTO_KMER_MAX_BYTES)
  bool fk_on = true;                  // f16x3 FC1 as a block-Karatsuba convolution (EXPECTO_FC1_KARATSUBA)
  int fk_role = 4;                    //   role of per-window forwards (EXPECTO_FC1_ROLE; 4 = direct FC1, the default; 0..3 Karatsuba)
  int fk_slice = 0;                   //   cap on the windows per Karatsuba FC1 launch on the segment path (EXPECTO_FC1K_SLICE;
                                      //   0: kFkSlicePerBatch x max_batch, one launch per chunk of the 200-window workload)
  bool fk_alt_inplace = false;        //   segment pairs: the alt FC1 as a masked pass of its own over the ref partial rows
                                      //   (EXPECTO_FC1K_ALT_INPLACE=1); default: alt rows of the ref launch, out of place
  bool onehot_as_codes = true;        // forward_onehot: exact one-hot input through the k-mer gather (EXPECTO_ONEHOT_CODES)
};

// One knob: its variable, its field (one of b / i / d), and for an int what it accepts: values
// below `floor` are raised to it (no refusal), then `ok` (if any) must hold or `refusal` is returned.
struct BelugaKnob {
  const char* name;
  bool BelugaKnobs::*b;
  int BelugaKnobs::*i;
  double BelugaKnobs::*d;
  int floor;
  bool (*ok)(int);
  const char* refusal;
};

namespace knob_detail {
using K = BelugaKnobs;
constexpr int kAny = std::numeric_limits<int>::min();
constexpr BelugaKnob flag(const char* n, bool K::*f) { return {n, f, nullptr, nullptr, kAny, nullptr, nullptr}; }
constexpr BelugaKnob num(const char* n, int K::*f, int floor = kAny, bool (*ok)(int) = nullptr, const char* why = nullptr) {
  return {n, nullptr, f, nullptr, floor, ok, why};
}
constexpr BelugaKnob real(const char* n, double K::*f) { return {n, nullptr, nullptr, f, kAny, nullptr, nullptr}; }
inline bool fc1_splits_ok(int v) { return v >= 1 && v <= 32 && kFc1KBlocks % v == 0; }
inline bool fc2_splits_ok(int v) { return v >= 1 && kFc2KBlocks % v == 0; }
inline bool role_ok(int v) { return v >= 0 && v <= 4; }
inline bool tri_ok(int v) { return v >= -1 && v <= 1; }
inline bool conv_tile_ok(int v) { return v == 0 || v == 256 || v == 384; }
}  // namespace knob_detail

// Every knob, once.  Values are read with atoi / atof; a flag is on for any nonzero integer.
// "same bits": the knob never changes an output bit; "parity": it picks how sums are formed.
inline constexpr BelugaKnob kBelugaKnobs[] = {
    // tuning knobs fixed per handle, so the split-K sums never depend on the batch
    knob_detail::num("EXPECTO_FC1_SPLITS", &BelugaKnobs::fc_splits, knob_detail::kAny, knob_detail::fc1_splits_ok,
                     "EXPECTO_FC1_SPLITS must divide 2120 and be <= 32"),
    knob_detail::num("EXPECTO_FC2_SPLITS", &BelugaKnobs::fc2_splits, knob_detail::kAny, knob_detail::fc2_splits_ok,
                     "EXPECTO_FC2_SPLITS must divide 63"),
    knob_detail::num("EXPECTO_FC2_ROWS", &BelugaKnobs::fc2_rows_env, 1),                 // same bits for any value
    knob_detail::real("EXPECTO_FC1_M_ORDER_MB", &BelugaKnobs::fc1_m_order_mb),           // same bits
    knob_detail::num("EXPECTO_FC1_ORDER", &BelugaKnobs::fc1_order),                      // same bits
    knob_detail::num("EXPECTO_FC1_M_GROUP", &BelugaKnobs::fc1_m_group, 1),               // same bits
    knob_detail::flag("EXPECTO_FC_WIDE", &BelugaKnobs::fc_wide),                         // same bits
    knob_detail::flag("EXPECTO_OVERLAP", &BelugaKnobs::overlap),                         // same bits
    knob_detail::flag("EXPECTO_POOL_ONE_PASS", &BelugaKnobs::pool_one_pass),             // same bits
    knob_detail::flag("EXPECTO_POOL_FUSED", &BelugaKnobs::pool_fused),                   // same bits
    knob_detail::flag("EXPECTO_FUSE_CONV1", &BelugaKnobs::fuse_conv1),                   // same bits
    knob_detail::flag("EXPECTO_CONV2_TABLE", &BelugaKnobs::kmer_on),                     // 0: conv2 on the MFMAs (parity)
    knob_detail::flag("EXPECTO_KMER_QUAD", &BelugaKnobs::kmer_quad),                     // 0: pair tables only (parity)
    knob_detail::real("EXPECTO_KMER_MAX_BYTES", &BelugaKnobs::kmer_max_bytes),
    knob_detail::flag("EXPECTO_ONEHOT_CODES", &BelugaKnobs::onehot_as_codes),            // parity
    knob_detail::flag("EXPECTO_FC1_KARATSUBA", &BelugaKnobs::fk_on),                     // parity
    knob_detail::num("EXPECTO_FC1K_SLICE", &BelugaKnobs::fk_slice, 1),                   // same bits
    knob_detail::num("EXPECTO_FC1_ROLE", &BelugaKnobs::fk_role, knob_detail::kAny, knob_detail::role_ok,
                     "EXPECTO_FC1_ROLE must be 0..4"),                                   // (tests)
    knob_detail::num("EXPECTO_SEG_CHUNK_WINDOWS", &BelugaKnobs::seg_chunk_windows),      // same bits
    knob_detail::flag("EXPECTO_SEG_MERGE_STRANDS", &BelugaKnobs::seg_merge_strands),     // same bits
    knob_detail::num("EXPECTO_CONV_NARROW", &BelugaKnobs::conv_narrow, knob_detail::kAny, knob_detail::tri_ok,
                     "EXPECTO_CONV_NARROW must be -1 (auto), 0 or 1"),                   // same bits
    knob_detail::num("EXPECTO_FC1_NARROW", &BelugaKnobs::fc1_narrow, knob_detail::kAny, knob_detail::tri_ok,
                     "EXPECTO_FC1_NARROW must be -1 (auto), 0 or 1"),                    // same bits
    knob_detail::flag("EXPECTO_CONV_EA", &BelugaKnobs::conv_ea),                         // same bits
    knob_detail::flag("EXPECTO_FC_SKINNY", &BelugaKnobs::fc_skinny),                     // same bits
    knob_detail::num("EXPECTO_CONV_TILE", &BelugaKnobs::conv_tile, knob_detail::kAny, knob_detail::conv_tile_ok,
                     "EXPECTO_CONV_TILE must be 0 (auto), 256 or 384"),                  // same bits
};

// A/B switches: read like the knobs, but no tuning knobs -- each keeps an earlier schedule of the
// library for comparisons inside one process (INTEGRATION.md lists them below the knob table).
inline constexpr BelugaKnob kBelugaSwitches[] = {
    knob_detail::flag("EXPECTO_FC1K_ALT_INPLACE", &BelugaKnobs::fk_alt_inplace),         // same bits
};

// Fills k from `get` (getenv's signature: the value of a variable, or null).  Returns null, or the
// refusal of the first knob in the table whose value is not accepted; k is then partly filled.
template <class Getenv>
const char* beluga_knobs_parse(BelugaKnobs& k, Getenv&& get) {
  for (const BelugaKnob& s : kBelugaKnobs) {
    const char* e = get(s.name);
    if (!e) continue;
    if (s.b) {
      k.*s.b = atoi(e) != 0;
    } else if (s.d) {
      k.*s.d = atof(e);
    } else {
      const int v = std::max(s.floor, atoi(e));
      if (s.ok && !s.ok(v)) return s.refusal;
      k.*s.i = v;
    }
  }
  for (const BelugaKnob& s : kBelugaSwitches)
    if (const char* e = get(s.name)) k.*s.b = atoi(e) != 0;
  return nullptr;
}

}  // namespace expecto
