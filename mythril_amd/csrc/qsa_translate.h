// qsa_translate.h — stack program (gprog.h) -> threaded code of the assembly interpreters
// (qsa.hip: P, preloaded variables; G, general), and the plans that go with it.  Host only: the
// translator sees the handler table and the model layout as plain data (QsaTable, ModelLayout),
// never the context that owns them, so it runs without a device.
#ifndef MQ_QSA_TRANSLATE_H
#define MQ_QSA_TRANSLATE_H
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gprog.h"
#include "qsa_table.h"
#include "tape_compiler.h"

namespace mq {

// words past the function entries that reads may touch (8 entries of the widest G table)
constexpr size_t kEntryPadWords = 512;
// the assembly interpreter keeps temps in LDS (2 KB per temp per wave, 4 waves per workgroup)
constexpr int kQsaMaxTemps = 16;

// Handler byte offset -> the 16-bit word field that encodes it: P / G handlers are 4-byte
// aligned (shift 2); the diagnostic G profile build aligns them to 8 bytes (shift 3, 512 KB reach)
inline uint32_t hword(int k, uint32_t off) { return off >> (k == 1 ? kQsaHandlerShiftG : 2); }
// P entries hold absolute handler addresses, so nothing in the kernel bounds P's handler area;
// the host's word -> kind table (QsaTable::kind_of, histograms) does: 2^18 four-byte words = 1 MB
// of handlers.  With the fused narrow handlers the last P handler starts 267 684 bytes (261 KB)
// behind the handler base.  A handler past the bound makes QsaTable::build return false: the
// assembly interpreters do not come up, nothing runs wrong.
constexpr uint32_t kQsaWordReachP = 1u << 18;

// The handler table of the assembly interpreters; k = 0 the P kernel, k = 1 the G kernel.
struct QsaTable {
  std::vector<uint32_t> off[2];          // byte offset of every handler from the handler base
  int index[2][QK_COUNT][kQsaStack][kQsaSel + 1];   // (kind, slot, selector + 1) -> handler, or -1
  // G kinds that wait for every vector load themselves (PUSH_MEMB, MEQK*, UF1*)
  bool vm_drain[QK_COUNT] = {};
  std::vector<uint8_t> data_words;       // G handler word -> inline data words that follow it
  uint32_t hbase_lo[2] = {0, 0};         // low 32 bits of each interpreter's handler base
  std::vector<int16_t> kind_of[2];       // handler word -> QsaKind (histograms)
  // Everything above from the generated handler keys (qsa_table.h) and, per interpreter, the
  // handlers' byte offsets and the low half of the handler base.  False: an offset is missing,
  // misaligned or out of the 16-bit word's reach, or base + offset leaves the base's 4 GB.
  bool build(const std::vector<uint32_t> (&offsets)[2], const uint32_t (&base_lo)[2]);
};

// Host copy of the model batch layout the translations and plans depend on.
struct ModelLayout {
  std::vector<uint32_t> var_off, var_nl;   // per variable: its first limb row, its limbs
  std::vector<uint16_t> var_width;
  // Bool variables as packed lane masks (G kernel PUSH_PKB): mask index of Bool variable v (-1: none)
  std::vector<int32_t> bmask_of_var;
  std::vector<mq_func_desc> funcs;
  int64_t entry_words_n = 0;   // words of function entries (G scans them with 32-bit offsets)
  // the all-zero row behind the last variable's rows
  uint32_t zero_row() const { return (uint32_t)(var_off.empty() ? 0 : var_off.back() + var_nl.back()); }
};

// The program the assembly interpreter k runs: G's stack has kQsaStackG slots, so a deeper
// program runs its spilled variant (tape_compiler.cpp CompiledTape::prog_g).
inline const std::vector<uint32_t>& qsa_prog(const CompiledTape& x, int k) {
  return (k == 1 && !x.prog_g.empty()) ? x.prog_g : x.prog;
}
inline int qsa_temps(const CompiledTape& x, int k) { return (k == 1 && !x.prog_g.empty()) ? x.n_temps_g : x.n_temps; }
inline int qsa_depth(const CompiledTape& x, int k) { return (k == 1 && !x.prog_g.empty()) ? x.depth_g : x.depth; }

// (the functions are documented at their definitions, qsa_translate.cpp)
void qsa_count(const QsaTable& qt, int k, const std::vector<uint32_t>& tr, std::vector<int64_t>& hist,
               std::vector<int64_t>* pairs);
bool qsa_translate(const QsaTable& qt, const ModelLayout& ml, int k, bool models, const CompiledTape& x,
                   std::vector<uint32_t>* out_p, std::vector<uint32_t>* extra_p, const std::vector<int>* gpre = nullptr,
                   const std::vector<int>* gstage = nullptr, bool g_bail = false);
bool qsa_translate_pf(const QsaTable& qt, const CompiledTape& x, std::vector<uint32_t>& out);
bool p_candidate(const CompiledTape& x);
void qsa_window_layout(const QsaTable& qt, std::vector<uint32_t>& prog);
uint32_t qsa_pack_program(const QsaTable& qt, std::vector<uint32_t>& out, size_t& pos, const std::vector<uint32_t>& prog);
std::vector<int64_t> count_pushes(const ModelLayout& ml, const std::vector<CompiledTape>& cts,
                                  const std::vector<char>* skip = nullptr);
void plan_stage(const ModelLayout& ml, const std::vector<int64_t>& pushes, const std::vector<int>* gpre, int temps,
                double wg_share, std::vector<int>& gstage, std::vector<uint32_t>& rows);

}  // namespace mq
#endif
