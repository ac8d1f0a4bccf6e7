// qs_types.h — the plain tables the host planners (fc_plan.cpp) fill and the flat-conjunction
// kernels (fc.hip) read.  No HIP header: host-only code includes this, qs_launch.h adds the
// argument blocks that hold device pointers and the launchers.
#ifndef MQ_QS_TYPES_H
#define MQ_QS_TYPES_H
#include <stdint.h>

namespace mq {

// Flat conjunctions (fc.hip, fc_plan.cpp fc_match): a tape or Bool column that is an AND of Bool
// model variables (negated or not) and comparisons of one variable with a constant.
struct FcCmpHead {    // (one 32-byte scalar load: all a variable of one or two limbs needs)
  uint32_t slot;      // LDS slot of the variable's limb 0 (limb l at slot + l; padded with zero rows)
  uint32_t nl;        // its limbs (1..8): <= 2 reads two slots, else eight
  uint32_t accept;    // bit 0: x < c, bit 1: x == c, bit 2: x > c (unsigned over the limbs)
  uint32_t pad;
  uint64_t c01;       // the constant's limbs 0-1 (sign bit flipped for a signed compare)
  uint64_t f01;       // XOR-ed into the variable's limbs 0-1: the sign bit of a signed compare
};
struct FcCmpTail {    // limbs 2-7 of a wider variable
  uint32_t c[6];
  uint32_t f[6];
};
struct alignas(16) FcCmp {
  FcCmpHead h;
  FcCmpTail t;
};
struct FcTape {
  uint32_t out;       // modes 0/1: tape index; mode 3: the Bool column's variable row
  int32_t mask_out;   // mode 3: its packed lane-mask index (-1: none, the 0/1 row is written)
  uint32_t mask_off;  // its Bool variables: FcArgs.mask_lds[mask_off ..] = 8 x LDS mask slot | negated,
  uint32_t n_mask;    //   n_mask of them, padded to a multiple of 16 with the last (bit 31: the
                      //   result is negated, an OR of atoms)
  uint32_t cmp_off;   // its compares: FcArgs.cmps[cmp_off ..]
  uint32_t n_cmp;
  uint32_t n_nodes;   // DAG nodes (metric)
  uint32_t alg_ops;   // SURVEY §8(d) algorithmic ops per model (metric)
};

// Two-phase flat conjunctions (fc.hip fca_kernel, fc_plan.cpp fca_plan), for tapes: the launch's
// distinct compares ("atoms") are evaluated once per 64-model tile into lane masks in LDS (model
// lanes), grouped by the variable they read (one read of its limbs per group), then every tape
// ANDs its atoms' and Bool variables' masks with one lane per tape.  A workgroup's LDS table per
// tile: entry 0 all ones, 1 .. n_smask the Bool masks, then the atoms; a list entry is a table
// index | negated << 31.
// Unary atoms (round 6): an atom may compare a constant with a UNARY function of its variable —
// a chain of at most kFcMaxXops constant-operand steps (the narrow / sign-extended column reads,
// shifts, extracts and divisions by small constants of C3's path conditions, instructions.py:
// 510-573).  Step k transforms the 8-limb value of width w_in (bits above it zero).
enum FcXcode : uint32_t {
  FX_SEXT = 1,     // p0 = result width
  FX_EXTRACT = 2,  // p0 = lo, p1 = result width
  FX_LSHR = 3,     // p0 = shift (>= w_in: 0)
  FX_SHL = 4,      // p0 = shift (>= w_in: 0)
  FX_ASHR = 5,     // p0 = shift (clamped to w_in - 1)
  FX_UREM = 6,     // p0 = divisor, 0 < d < 2^21
  FX_UDIV = 7,     // p0 = divisor
  FX_SMOD = 8,     // p0 = |divisor|, p1 = divisor negative (SMT-LIB bvsmod)
  FX_SREM = 9,     // p0 = |divisor|, p1 = divisor negative (bvsrem)
  FX_SDIV = 10     // p0 = |divisor|, p1 = divisor negative (bvsdiv)
};
constexpr int kFcMaxXops = 3;
struct FcXop {
  uint32_t code;   // FcXcode | w_in << 8
  uint32_t p0, p1, p2;
};
struct FcXf {      // per atom (FcaArgs.xfs, parallel to atoms); n = 0: the variable itself
  uint32_t n, pad[3];
  FcXop op[kFcMaxXops];
};
struct FcaGroup {
  uint32_t rows[8];   // the variable's limb rows (nl <= 2: rows[0..1]; else 8, the zero row past nl)
  uint32_t first;     // its atoms: atoms[first .. first + count)
  uint32_t count;
  uint32_t nl;
  uint32_t pad;
};

}  // namespace mq
#endif
