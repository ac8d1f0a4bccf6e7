// fc_plan.h — host planners of the flat-conjunction kernels (fc.hip) and of G's column groups:
// which programs are flat conjunctions (fc_match), the kernels' tables (fc_plan, fca_plan) and a
// column level's wave groups (balance_groups).  Host only: they see the model layout as plain
// data (ModelLayout), never the context, and fill the plain tables of qs_types.h.
#ifndef MQ_FC_PLAN_H
#define MQ_FC_PLAN_H
#include <stdint.h>
#include <functional>
#include <utility>
#include <vector>
#include "qs_types.h"
#include "qsa_translate.h"

namespace mq {

// A flat conjunction (fc.hip): the stack program of x, run abstractly, leaves an AND of Bool
// variables (negated or not) and compares of one model variable of at most 256 bits with a
// constant; temps, arithmetic and anything else do not match.  A Bool variable without a lane-mask
// index is a compare of its 0/1 row with 1.  Appends its masks (index | negated << 31) and
// compares (FcCmpH: the variable's first row and limbs, the predicate as an accept mask over
// (x < c, x == c, x > c), the constant; signed compares have the sign bit flipped) to the lists.
struct FcCmpH {
  uint32_t row, nl, accept;
  uint32_t c[8], f[8];
  uint32_t src_nl = 0;   // limbs of the compared variable's rows (0: nl; fewer when it was zero-extended)
  uint32_t nx = 0;       // unary atoms (fca only): the variable's transform, nx steps
  FcXop xf[kFcMaxXops] = {};
};
// accept masks: bit 0 x < c, bit 1 x == c, bit 2 x > c
constexpr uint32_t kAccEq = 2, kAccNe = 5, kAccLt = 1, kAccLe = 3, kAccGt = 4, kAccGe = 6;
// LDS budget of the flat-conjunction kernel's staging, per tile (fc.hip stages FC_TILES = 4
// tiles a workgroup): rows of 256 B (40 KB for 4 tiles) and masks of 8 B (8 KB for 4 tiles);
// only what a launch uses is allocated (C4's tapes: ~5 KB)
constexpr int kFcStageRows = 40;
constexpr int kFcStageMasks = 256;

bool fc_match(const ModelLayout& ml, const CompiledTape& x, std::vector<uint32_t>& masks, std::vector<FcCmpH>& cmps,
              bool* neg = nullptr, bool unary = false);

// The flat-conjunction kernel's tables for the tapes (or columns) `cand` of the lists `fm` / `fq`
// (fc_match): the compared variables and the masks the most compares / tapes read are staged in
// LDS within the budgets; a candidate reading one that is not staged is dropped from `cand`'s
// kernel (keep[i] = 0: it stays on the interpreter).  out_of(i) and mask_out(i) give FcTape.out /
// .mask_out, nodes_ops(i) its metric words.
struct FcPlan {
  std::vector<FcTape> tapes;
  std::vector<uint32_t> mask_lds;
  std::vector<FcCmp> cmps;
  std::vector<uint32_t> stage_rows, stage_masks;
  std::vector<unsigned long long> prefix;
};
void fc_plan(const ModelLayout& ml, const std::vector<std::vector<uint32_t>>& fm, const std::vector<std::vector<FcCmpH>>& fq,
             const std::vector<char>& negated, std::vector<char>& keep, const std::function<uint32_t(size_t)>& out_of,
             const std::function<int32_t(size_t)>& mask_out,
             const std::function<std::pair<uint32_t, uint32_t>(size_t)>& nodes_ops, FcPlan& P);

struct FcaPlanSeg {   // one fca_kernel launch (fca_plan)
  int atom_off, n_atoms, group_off, n_groups, tape_first, n_tapes, chunk_first, smask_off, n_smask;
};
// The two-phase kernel's tables for the tapes `keep` of fm / fq (fca_kernel).  Tapes are taken
// in order into launches ("segments") of at most kFcaMaxAtoms distinct compares ("atoms": a
// compare and its negation are one atom, accept canonicalised to {1, 2, 3} and the negation moved
// into the list entry) and kFcStageMasks distinct Bool masks; a segment's atoms are ordered by
// the variable they read (one group per variable: its limbs are loaded once per tile).
struct FcaPlan {
  std::vector<FcCmp> atoms;
  std::vector<FcXf> xfs;   // parallel to atoms
  bool any_xf = false;     // some atom has a unary transform (else the launches pass xfs = nullptr)
  std::vector<FcaGroup> groups;
  std::vector<uint32_t> lists, chunk_off, tape_out, metric, stage_masks;
  std::vector<int32_t> col_mask;   // (columns: per kept column its lane-mask index)
  std::vector<FcaPlanSeg> segs;
  // one dummy element into every table a launch may find empty: an upload is never of zero bytes
  void pad_empty() {
    if (stage_masks.empty()) stage_masks.push_back(0);
    if (atoms.empty()) atoms.push_back(FcCmp{});
    if (xfs.empty()) xfs.push_back(FcXf{});
    if (groups.empty()) groups.push_back(FcaGroup{});
    if (lists.empty()) lists.push_back(0);
  }
};
constexpr int kFcaMaxAtoms = 1024;   // 32 KB of LDS masks for the 4 tiles of a workgroup
constexpr int kFcaGroupAtoms = 16;   // (C4 fca: 4 -> 213 us, 8 -> 196, 16 -> 186, 32 -> 199)
void fca_plan(const ModelLayout& ml, const std::vector<std::vector<uint32_t>>& fm, const std::vector<std::vector<FcCmpH>>& fq,
              const std::vector<char>& negated, std::vector<char>& keep, const std::function<uint32_t(size_t)>& out_of,
              const std::function<std::pair<uint32_t, uint32_t>(size_t)>& nodes_ops, FcaPlan& P,
              const std::function<int32_t(size_t)>& mask_out = nullptr);

// (documented at their definitions, fc_plan.cpp)
double g_cost(const CompiledTape& x);
void balance_groups(const std::vector<CompiledTape>& ct, std::vector<int>& idx, int tpg, std::vector<uint32_t>& tab);

}  // namespace mq
#endif
