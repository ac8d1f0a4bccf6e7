// qs_launch.h — kernel argument blocks and launchers shared by mq_api.cpp and the kernels; the plain
// tables the host planners fill are qs_types.h's.
#ifndef MQ_QS_LAUNCH_H
#define MQ_QS_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gprog.h"
#include "qs_types.h"

namespace mq {

// Work counters (pairs evaluated, node-evals, algorithmic ops): kCounterSlots slots of
// kCounterStride u64 (128 B apart), a wave adds into slot (workgroup id mod kCounterSlots) so a
// launch of 10^6 waves does not serialise on one cache line; the host sums the slots.
constexpr int kCounterSlots = 256;
constexpr int kCounterStride = 16;

// device view of one model function (UF or as-array interpretation)
struct FuncDev {
  uint32_t arity;
  uint32_t nl_a0, nl_a1, nl_res;
  uint32_t stride;      // words per entry
  uint32_t dense_e;     // > 0: also held as dense slots (G lookups): entry slots per model
  int64_t entry_base;   // word offset of entry 0 in entry_words
  int64_t ptr_base;     // offset of row pointers [M+1] in entry_ptr
  int64_t else_base;    // word offset of the SoA else block: else_words[else_base + limb*M + m]
  // dense slots (dense_e > 0): key limb l of entry slot e of model m at
  // dense_words[dense_base + (e * nl_a0 + l) * M + m], value limb l at
  // dense_words[dense_base + (dense_e * nl_a0 + e * nl_res + l) * M + m]; a model's entries keep
  // their order, slots past its count are never read (the count is entry_ptr's)
  int64_t dense_base;
};
static_assert(sizeof(FuncDev) == 56, "FuncDev layout (gen_qsa.py sub_uf1 reads it)");

struct KArgs {
  // tapes
  const GDesc* descs;
  int n_desc;
  int tapes_per_group;
  const uint32_t* prog;
  const uint32_t* consts;
  const uint32_t* tape_consts;  // unused on host; kept for layout stability
  // models
  const uint32_t* vars;
  const uint32_t* var_off;
  const uint32_t* var_nl;
  int n_vars;
  int n_funcs;
  const FuncDev* funcs;
  const int64_t* entry_ptr;
  const uint32_t* entry_words;
  const uint32_t* else_words;
  int64_t M;
  int64_t index_base;
  // outputs
  int32_t* best;                 // first-hit accumulator (global index, INT32_MAX = none)
  uint8_t* verdicts;             // verdict mode: [tape][M] bytes
  unsigned long long* counters;  // [slot][0] pairs evaluated, [1] node-evals, [2] algorithmic ops
  int tmp_words_per_wave;        // temp words per wave (slot, limb, lane)
  int early_exit;
  uint32_t* scratch;             // per-wave temp slots in HBM: [gridDim.x][tmp_words_per_wave]
  int64_t tiles;                 // model tiles of 64 (one wave = one workgroup)
  int64_t n_items;               // tiles x tape groups; workgroups stride over them
  int grid;                      // workgroups launched (persistent, <= n_items)
  int stack_slots;               // LDS operand-stack slots per wave (max program depth)
  int mode;                      // 0 first hit, 1 verdicts, 2 columns (GDesc.tape = target var)
};

// argument block of the assembly interpreter (layout fixed by gen_qsa.py's prologue)
struct QArgs {
  const void* descs;             // 0x00 GDesc[] (prog_off indexes the QSA program words)
  const void* prog;              // 0x08
  const void* consts;            // 0x10
  const void* vars;              // 0x18
  int32_t* best;                 // 0x20
  unsigned long long* counters;  // 0x28
  uint8_t* verdicts;             // 0x30
  uint32_t* table_out;           // 0x38 (mode 2)
  uint32_t M;                    // 0x40
  uint32_t index_base;           // 0x44
  uint32_t n_desc;               // 0x48
  uint32_t tapes_per_group;      // 0x4c
  uint32_t early_exit;           // 0x50
  uint32_t mode;                 // 0x54: 0 first-hit, 1 verdicts, 2 dump handler offsets
  uint32_t lds_wave_bytes;       // 0x58
  uint32_t pad;                  // 0x5c
  uint32_t var_row[64];          // 0x60: limb row of var v limb l (v < 8), or the zero row
  const void* funcs;             // 0x160 FuncDev[] (G kernel: UF1 lookups)
  const void* entry_ptr;         // 0x168
  const void* entry_words;       // 0x170
  const void* else_words;        // 0x178
  uint32_t n_funcs;              // 0x180
  uint32_t n_stage;              // 0x184 G: model rows staged in LDS per workgroup (multiple of 8)
  uint32_t stage_base;           // 0x188 G: LDS byte offset of the staged rows
  uint32_t bool_rows;            // 0x18c G mode 3: also write Bool columns' 0/1 rows (a C++ kernel reads them)
  const uint32_t* stage_rows;    // 0x190 G: global row of each staged slot
  const uint64_t* bool_masks;    // 0x198 G: packed Bool rows, [tile][n_bool_masks] lane masks
  uint32_t n_bool_masks;         // 0x1a0
  uint32_t reserved_1a4;         // 0x1a4 (unused; keeps the layout the generated code addresses)
  unsigned long long* prof_out;  // 0x1a8 G profile build only: (cycles, count) per handler kind
  const uint32_t* dense_words;   // 0x1b0 G: dense lookup slots (FuncDev dense_base / dense_e)
  // P, low-limb prefilter (gen_qsa.py pf_frame / alive_scan).  alive: [ceil(M / 64)][alive_words]
  // bits, bit (desc & 31) of word desc >> 5 of a block's row = "tape desc may hold for a model of
  // the block".  Mode 4 sets the bits of the blocks its narrow programs do not clear; mode 0 with
  // a non-null alive runs, per 64-model block, only the tapes whose bit is set there or in
  // alive_static (the descriptors without a prefilter program).  Null: the launch is unfiltered.
  uint32_t* alive;               // 0x1b8
  const uint32_t* alive_static;  // 0x1c0 [alive_words]
  const void* pf_descs;          // 0x1c8 mode 4: GDesc[] parallel to descs (prog_len 0: no prefilter)
  uint32_t alive_words;          // 0x1d0
  uint32_t reserved_1d4;         // 0x1d4
};
static_assert(sizeof(void*) == 8, "64-bit");
static_assert(__builtin_offsetof(QArgs, M) == 0x40, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, var_row) == 0x60, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, funcs) == 0x160, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, n_funcs) == 0x180, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, n_stage) == 0x184, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, bool_rows) == 0x18c, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, stage_rows) == 0x190, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, bool_masks) == 0x198, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, n_bool_masks) == 0x1a0, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, reserved_1a4) == 0x1a4, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, prof_out) == 0x1a8, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, dense_words) == 0x1b0, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, alive) == 0x1b8, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, alive_static) == 0x1c0, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, pf_descs) == 0x1c8, "QArgs layout");
static_assert(__builtin_offsetof(QArgs, alive_words) == 0x1d0, "QArgs layout");

// variant 0 = P (preloaded variables, qsa_kernel), 1 = G (general, qsg_kernel)
hipError_t launch_qsa(int variant, const QArgs* d_args, unsigned gx, unsigned gy, size_t lds, hipStream_t st);
hipError_t launch_qs(const KArgs& a, int L, bool keccak, bool verdict, hipStream_t st);
hipError_t launch_columns(const KArgs& a, int L, bool keccak, hipStream_t st);
hipError_t launch_init_best(int32_t* best, int n, hipStream_t st);
hipError_t launch_mask_rows(uint32_t* vars, const uint32_t* rowmask, int64_t rows, int64_t M, hipStream_t st);
// masks[tile * n_masks + j] = lane mask of (vars[rows[j]][64 * tile + i] != 0), for j in list[0..n)
// (list == nullptr: j = 0..n-1)
hipError_t launch_pack_bool(const uint32_t* vars, uint64_t* masks, const uint32_t* rows, const int32_t* list, int n,
                            int n_masks, int64_t M, hipStream_t st);
// Derived upload (mq_models_upload_derived): the variable rows [rows, M = n_base + K] written on
// the device.  Column m < n_base is base[row * n_base + m]; column n_base + k is the column of
// src[k] (-1: zeros) with the patches of k's block (block_start: [n_blocks + 1], patch_ptr into
// patches) applied, then (a second launch on the same stream, so a floor sees every patched limb
// of its variable) the block's floors.  RowPatch / RowFloor are mq.h's mq_row_patch / mq_row_floor.
struct RowPatch {
  uint32_t row, keep, bits;
};
struct RowFloor {
  uint32_t row0, n_limbs, minimum;
};
hipError_t launch_derive_rows(uint32_t* vars, const uint32_t* base, const int32_t* src, const int64_t* block_start,
                              const int64_t* patch_ptr, const RowPatch* patches, const int64_t* floor_ptr,
                              const RowFloor* floors, int64_t n_floors, int64_t n_base, int64_t K, int64_t rows,
                              int32_t n_blocks, hipStream_t st);
// Derived function tables (mq_models_upload_derived_tables): the CSR row pointers, entry words,
// SoA else values and dense slots of all M = n_base + K models written on the device from the
// base models' tables and each block's additions, after the rows are derived and masked (an added
// entry's value is the model's resident limbs of a variable).  Model m < n_base keeps base model
// m's entries; derived model k of block j has the block's additions for the function first, in
// list order, then the entries of base model src[k] (none for -1; else value 0), then (n_sites > 0)
// one entry per active keccak site of the block that appends to the function, in site order.
struct TableAdd {   // mq.h's mq_table_add
  int32_t func, var;
  int64_t key_off;
};
struct TableDerive {
  const FuncDev* funcs;          // the OUTPUT layout (ptr_base, entry_base, else_base, dense_*), [n_funcs]
  const int64_t* b_ptr;          // base CSR rows [n_funcs][n_base + 1], each from 0
  const int64_t* b_base;         // [2 * n_funcs]: word offset of f's entries in b_entries, of its else values in b_else
  const uint32_t* b_entries;     // base entries, stride words each
  const uint32_t* b_else;        // base else values, AoS: b_else[b_base[2f+1] + m * nl_res + l]
  const int32_t* src;            // [K]
  const int64_t* block_start;    // [n_blocks + 1]
  const int64_t* add_ptr;        // [n_blocks + 1] into adds
  const TableAdd* adds;
  const int32_t* add_cnt;        // [n_funcs][n_blocks]: additions of block j to function f
  const uint32_t* keys;          // key pool: an addition's constant key words at key_off
  const uint32_t* vars;          // the resident rows [rows][M], masked
  const uint32_t* var_off;       // [n_vars] first row of a variable
  int64_t* entry_ptr;
  uint32_t* entry_words;
  uint32_t* else_words;
  uint32_t* dense_words;         // zeroed by the caller
  int64_t n_base, K;
  int32_t n_blocks, n_funcs;
  // keccak sites (mq_models_upload_derived_keccak; n_sites == 0: none, the pointers unused): a
  // derived model's third segment, behind its base model's entries
  int32_t n_sites;
  const struct KsSite* ks_sites;
  const struct KcMapEntry* ks_words;   // a site's input limbs: a row, or row == ~0u: the constant `value`
  const struct KsInv* ks_inv;
  const uint64_t* ks_active;     // [n_blocks] sites active in a block
  const uint64_t* ks_fmask;      // [n_funcs] sites that append an entry to function f
  const int32_t* ks_cnt;         // [n_funcs][n_blocks]: popcount(ks_active[j] & ks_fmask[f])
  const uint32_t* ks_v;          // the sites' images, SoA [slot][limb 0..7][K] (derive_keccak_sites_kernel)
  uint64_t ks_union;             // sites active in some block: only those have a slot in ks_v (ks_slot)
};
// slot of site `si` in the image scratch: its rank among the sites that are active in some block
__device__ __forceinline__ int ks_slot(uint64_t ks_union, int si) { return __popcll(ks_union & ((1ull << si) - 1ull)); }
// mq.h's mq_keccak_site / mq_keccak_inverse / mq_keccak_collision (mq_keccak_word is KcMapEntry)
struct KsSite {
  int32_t func;
  uint32_t n_words;
  int64_t map_off;
  int32_t inv_off, n_inv;
  int32_t coll_off, n_coll;
  uint32_t b, pad;
  uint32_t base[8];
};
struct KsInv {
  int32_t func;
  uint32_t lo_word;
};
struct KsColl {
  int32_t var, pad;
  int64_t key_off;
};
// One thread per (derived model, site), after the rows are derived, floored and masked: v of every
// active pair into v_out[(ks_slot(live, site) * 8 + limb) * K + k], `live` the union of the blocks'
// masks, v_out 8 * popcount(live) * K words (inactive pairs are left unwritten, never read)
hipError_t launch_derive_keccak_sites(const KsSite* sites, int n_sites, const struct KcMapEntry* words, const KsColl* coll,
                                      const uint32_t* keys, const uint64_t* active, uint64_t live, const int64_t* block_start,
                                      int32_t n_blocks, const uint32_t* vars, const uint32_t* var_off, int64_t n_base,
                                      int64_t K, uint32_t* v_out, hipStream_t st);

// the last block whose start is <= k (empty blocks before it are skipped)
__device__ __forceinline__ int derive_block_of(const int64_t* block_start, int n_blocks, int64_t k) {
  int lo = 0, hi = n_blocks;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_start[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
// threads of the one workgroup per function that scans the entry counts into entry_ptr: thread t
// owns models [t * chunk, (t + 1) * chunk), chunk = ceil(M / kTableScanThreads)
constexpr int kTableScanThreads = 256;
// max_words: the most entry words (entries * stride) any function holds (sizes the entries grid)
hipError_t launch_derive_tables(const TableDerive& a, int64_t max_words, bool any_dense, hipStream_t st);
hipError_t launch_finalize_best(int32_t* best, const uint8_t* unsupported, int n, hipStream_t st);
hipError_t launch_keccak(const uint8_t* data, const int64_t* offsets, int n, uint8_t* out, hipStream_t st);

// Keccak columns (mq_api.cpp kc_*): a hoisted column that is exactly keccak256(concat of model
// variables and constants), evaluated by a dedicated keccak-f[1600] kernel, one model per lane.
// Message word i (little-endian u32 of the big-endian message bytes) = bswap32 of map entry i:
// a variable row (vars[row * M + m]) or, with row == ~0u, the constant word `value`.
struct KcMapEntry {
  uint32_t row;
  uint32_t value;
};
struct KcCol {
  uint32_t map_off;     // first map entry of the column
  uint32_t nwords;      // message words (<= 64: at most 2048 bits, two 136-byte blocks)
  uint32_t target_row;  // first of the 8 rows of the column's variable
  uint32_t n_nodes;     // DAG nodes of the column program (metric; + its predicates')
  uint32_t alg_ops;     // SURVEY §8(d) algorithmic ops of the program (metric; + its predicates')
  uint32_t pred_off;    // its predicate columns (KcPred) evaluated from the digest in registers
  uint32_t n_pred;
  uint32_t pad;
};
// A Bool column comparing a keccak column h with a constant (lower.py keccak_predicates,
// mq_api.cpp kp_match): evaluated by the keccak column kernel right after h
enum KcPredKind : uint32_t { KP_LT = 0, KP_GT = 1, KP_GE = 2, KP_LE = 3, KP_EQ = 4, KP_LOWZ = 5 };
struct KcPred {
  uint32_t kind;        // h < c, h > c, h >= c, h <= c, h == c, low `bits` bits of h zero
  uint32_t bits;        // KP_LOWZ: number of low bits
  uint32_t row;         // the Bool column's variable row (0/1 per model)
  int32_t mask;         // its packed lane-mask index (-1: none)
  uint32_t c[8];        // the constant, limbs little-endian
};
hipError_t launch_keccak_columns(const KcCol* cols, int n_cols, const KcMapEntry* map, const KcPred* preds,
                                 uint32_t* vars, int64_t M, unsigned long long* counters, uint64_t* bool_masks,
                                 int n_bool_masks, int bool_rows, hipStream_t st);

// Bit-gather columns (cw.hip, mq_api.cpp cw_compile): a hoisted column whose value is model
// variable bits and constants, runs of bits optionally gated by `i <s size` (one 256-bit size
// variable per column).  Output limb `limb` = const_or | OR over its slots of
// (((vars[row] >> sb) & mask) << db), a slot whose gate fails giving 0; chunks of one limb are
// consecutive, the last one with store = 1.
struct CwSlot {
  uint32_t row;     // the variable row (a zero row, mask 0: an empty slot)
  uint32_t mask;
  uint32_t shifts;  // sb | db << 8
  uint32_t gate;    // i (< 2^31): the slot counts when i <s size; ~0u: ungated
};
struct CwChunk {
  CwSlot s[4];
  uint32_t limb, store, const_or, pad;
};
struct CwCol {
  uint32_t chunk_off, n_chunks;
  uint32_t target_row;  // limb 0 row of the column's variable
  uint32_t size_row;    // limb 0 row of the size variable (~0u: no gated slots)
  uint32_t n_nodes, alg_ops;   // of the column program (metric)
  uint32_t pad[2];
};
hipError_t launch_cw_columns(const CwCol* cols, int n_cols, const CwChunk* chunks, uint32_t* vars, int64_t M,
                             unsigned long long* counters, hipStream_t st);

// Flat conjunctions (fc.hip fc_kernel; the tables are qs_types.h's)
struct FcArgs {
  const FcTape* tapes;
  int n;                         // tapes / columns of the launch
  int tpg;                       // per wave (a workgroup's 4 waves take 4 groups of one tile)
  const uint32_t* mask_lds;
  const FcCmp* cmps;
  const uint32_t* vars;
  const uint64_t* bool_masks;    // [tile][n_bool_masks] packed Bool rows (read)
  uint64_t* bool_masks_out;      // mode 3: the same array, the level's columns written
  uint32_t* vars_out;            // mode 3: 0/1 rows
  int n_bool_masks;
  int mode;                      // 0 first hit, 1 verdict bytes, 3 Bool columns
  int early_exit;
  int bool_rows;                 // mode 3: also write the 0/1 row of a column with a mask index
  int64_t M;
  int64_t index_base;
  int32_t* best;
  uint8_t* verdicts;             // mode 1: [tape][M] bytes
  unsigned long long* counters;
  const uint32_t* stage_rows;    // variable rows staged in LDS per workgroup, slot order
  int n_stage;
  const uint32_t* stage_masks;   // mask indices staged in LDS per workgroup (after the rows)
  int n_smask;
  const unsigned long long* prefix;   // [2 (n + 1)]: running sums of n_nodes, alg_ops
};
// fc_kernel's by-value block (the read-only tables are separate __restrict__ arguments)
struct FcRun {
  int n, tpg, n_bool_masks, mode, early_exit, bool_rows;
  int64_t M, index_base;
  int32_t* best;
  uint8_t* verdicts;
  uint64_t* masks_out;
  uint32_t* vars_out;
  unsigned long long* counters;
  int n_stage, n_smask;
  const unsigned long long* prefix;
};
hipError_t launch_fc(const FcArgs& a, hipStream_t st);

// Two-phase flat conjunctions (fc.hip fca_kernel; the tables are qs_types.h's)
struct FcaArgs {
  int n;                          // tapes
  int n_atoms;
  int n_groups;
  const FcaGroup* groups;
  const FcCmp* atoms;             // accept in {1, 2, 3} (x < c, x == c, x <= c); negations in the lists
  const FcXf* xfs;                // per atom: its unary transform (n = 0: none); groups with one have nl = 8;
                                  // nullptr: no unary atom (the kernel without the transforms)
  const uint32_t* lists;          // chunk c of 64 tapes: kmax(c) entries x 64 lanes, k-major, from chunk_off[c]
  const uint32_t* chunk_off;      // [n_chunks + 1]: kmax(c) = (chunk_off[c + 1] - chunk_off[c]) / 64
  const uint32_t* tape_out;       // per tape: its best / verdict row | negated result << 31
  const uint32_t* tape_metric;    // per tape: n_nodes, alg_ops
  const uint32_t* vars;
  const uint64_t* bool_masks;
  int n_bool_masks;
  int mode;                       // 0 first hit, 1 verdict bytes, 3 Bool columns (tape_out = the column's row)
  int early_exit;
  int64_t M;
  int64_t index_base;
  int32_t* best;
  uint8_t* verdicts;
  unsigned long long* counters;
  const int32_t* col_mask;        // mode 3: per column its packed lane-mask index (-1: none, the 0/1 row is written)
  uint64_t* bool_masks_out;       // mode 3: the same array as bool_masks, the level's columns written
  uint32_t* vars_out;             // mode 3: 0/1 rows
  int bool_rows;                  // mode 3: also write the 0/1 row of a column with a mask index
  const uint32_t* stage_masks;    // the Bool mask indices of table entries 1 .. n_smask
  int n_smask;
};
hipError_t launch_fca(const FcaArgs& a, hipStream_t st);

}  // namespace mq
#endif
