// pf_translate_check — the low-limb prefilter translation (qsa_translate.cpp qsa_translate_pf) on a
// CPU: compiles a corpus of tape batches (the format of planner_check), translates every tape's
// prefilter program against a synthetic handler table (handler h at byte offset h << 2, base 0)
// and writes each entry as (kind name, slot, variable, immediate, third word).  Links
// tape_compiler.cpp and qsa_translate.cpp only; exit status 1 if a translation does not end on END
// or does not repeat.
//
//   pf_translate_check CORPUS [KIND]
//
// KIND: a handler kind taken out of the table before translating (the fallback to unfused entries).
// MQ_PF_FUSE is read by the translator itself.
//
// Output: "key KIND d v" for every P handler of qsa_table.h, then per batch "batch NAME" and per
// tape "tape T", "prog WORDS" (prog_pf, hex) and "pf N" followed by N lines "e KIND d v IMM W3"
// (N = 0: no prefilter program, or it does not translate).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../mythril_amd/csrc/qsa_translate.h"

using namespace mq;

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) return std::fprintf(stderr, "usage: pf_translate_check CORPUS [KIND]\n"), 2;
  std::ifstream in(argv[1]);
  if (!in) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  QsaTable qt;
  {
    std::vector<uint32_t> off[2];
    const uint32_t base[2] = {0, 0};
    for (int h = 0; h < kQsaHandlersP; h++) off[0].push_back((uint32_t)h << 2);
    for (int h = 0; h < kQsaHandlersG; h++) off[1].push_back((uint32_t)h << kQsaHandlerShiftG);
    if (!qt.build(off, base)) return std::fprintf(stderr, "the synthetic handler table is not valid\n"), 1;
  }
  if (argc == 3) {
    int drop = -1;
    for (int q = 0; q < QK_COUNT; q++)
      if (!std::strcmp(kQsaKindNames[q], argv[2])) drop = q;
    if (drop < 0) return std::fprintf(stderr, "no handler kind %s\n", argv[2]), 2;
    for (int d = 0; d < kQsaStack; d++)
      for (int v = 0; v <= kQsaSel; v++) qt.index[0][drop][d][v] = -1;
  }
  for (int h = 0; h < kQsaHandlersP; h++)
    std::printf("key %s %d %d\n", kQsaKindNames[kQsaHandlerKeysP[h].kind], kQsaHandlerKeysP[h].d, kQsaHandlerKeysP[h].v);

  int failures = 0;
  std::string word, name;
  while (in >> word) {
    int64_t n_vars, n_funcs, entry_words_n, n_tapes, n_nodes, n_consts;
    if (word != "batch" || !(in >> name >> n_vars >> n_funcs >> entry_words_n >> n_tapes >> n_nodes >> n_consts))
      return std::fprintf(stderr, "malformed batch header\n"), 2;
    for (int64_t i = 0; i < n_vars + 4 * n_funcs; i++) {   // (the layout plays no part here)
      unsigned skip;
      in >> skip;
    }
    std::vector<int64_t> offsets(n_tapes + 1);
    for (auto& o : offsets) in >> o;
    std::vector<mq_node> nodes(n_nodes);
    for (auto& n : nodes) {
      unsigned op, w;
      in >> op >> w >> n.a >> n.b >> n.c;
      n.op = (uint16_t)op;
      n.width = (uint16_t)w;
    }
    std::vector<uint32_t> consts(n_consts);
    for (auto& c : consts) in >> c;
    if (!in) return std::fprintf(stderr, "batch %s is cut short\n", name.c_str()), 2;
    consts.resize(consts.size() + 1, 0);
    mq_tape_batch tb{(int32_t)n_tapes, offsets.data(), nodes.data(), consts.data(), n_consts};
    std::printf("batch %s\n", name.c_str());
    CompileLimits lim;
    lim.g_depth = kQsaStackG;
    for (int32_t t = 0; t < n_tapes; t++) {
      const CompiledTape x = compile_tape(&tb, t, lim);
      std::printf("tape %d\nprog", t);
      for (uint32_t w : x.prog_pf) std::printf(" %x", w);
      std::printf("\n");
      std::vector<uint32_t> pf, pf2;
      const bool ok = x.supported && !x.prog_pf.empty() && qsa_translate_pf(qt, x, pf);
      if (ok && (!qsa_translate_pf(qt, x, pf2) || pf2 != pf)) {
        std::fprintf(stderr, "FAIL %s tape %d: a second translation differs\n", name.c_str(), t);
        failures++;
      }
      if (!x.prog_pf.empty() && !ok) {   // (every narrow program of the compiler fits the mode)
        std::fprintf(stderr, "FAIL %s tape %d: the prefilter program does not translate\n", name.c_str(), t);
        failures++;
      }
      std::printf("pf %zu\n", ok ? pf.size() / 3 : (size_t)0);
      if (!ok) continue;
      if (pf.size() % 3) failures++;
      for (size_t i = 0; i + 2 < pf.size(); i += 3) {
        const uint32_t h = pf[i] >> 2;
        if ((pf[i] & 3) || h >= (uint32_t)kQsaHandlersP) {
          std::fprintf(stderr, "FAIL %s tape %d: entry %zu is no handler\n", name.c_str(), t, i / 3);
          failures++;
          std::printf("e ? 0 0 0 0\n");
          continue;
        }
        const QsaHandlerKey& k = kQsaHandlerKeysP[h];
        std::printf("e %s %d %d %u %u\n", kQsaKindNames[k.kind], k.d, k.v, pf[i + 1], pf[i + 2]);
        if ((k.kind == QK_END) != (i + 3 == pf.size())) {
          std::fprintf(stderr, "FAIL %s tape %d: END is not exactly the last entry\n", name.c_str(), t);
          failures++;
        }
      }
    }
  }
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
