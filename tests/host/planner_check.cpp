// planner_check — the host planners on a CPU: compiles a corpus of tape batches, translates every
// tape for both assembly interpreters against a synthetic handler table (handler h at byte
// offset h << shift, base 0) and the batch's model layout, runs the flat-conjunction planners,
// writes what they made as text and checks the structure of every translation itself.  A last
// batch, `handbuilt`, is not read but made here (bail_behind_push).
// Links tape_compiler.cpp, qsa_translate.cpp and fc_plan.cpp only; exit status 1 if a check fails.
//
//   planner_check CORPUS
//
// CORPUS is whitespace-separated numbers, one record per batch:
//   batch NAME n_vars n_funcs entry_words_n n_tapes n_nodes n_consts
//   n_vars widths | n_funcs x (arity result_width arg_width0 arg_width1) | n_tapes + 1 offsets |
//   n_nodes x (op width a b c) | n_consts words
// Variable rows follow the upload's rule: limbs(width) rows each in order, the i-th Bool variable
// has lane-mask index i.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../mythril_amd/csrc/fc_plan.h"
#include "../../mythril_amd/csrc/qsa_translate.h"

using namespace mq;

static int g_failures = 0;
static std::string g_where;
static void fail(const std::string& what) {
  std::fprintf(stderr, "FAIL %s: %s\n", g_where.c_str(), what.c_str());
  g_failures++;
}

static int kind_at(const QsaTable& qt, int k, uint32_t w) {
  const uint32_t key = k == 0 ? ((w - qt.hbase_lo[0]) >> 2) & 0xFFFFu : w & 0xFFFFu;
  return qt.kind_of[k][key];
}

// Walk a translation handler by handler (P: three words an entry; G: a word and its inline data;
// `blocks`: G after qsa_window_layout, where REFILL continues at the next 64-word block, no group
// may straddle a block and END padding fills the last one).  It must end exactly on END / END_V.
static bool walk(const QsaTable& qt, int k, const std::vector<uint32_t>& tr, bool blocks, std::vector<int>* kinds) {
  size_t i = 0;
  while (i < tr.size()) {
    const int kind = kind_at(qt, k, tr[i]);
    if (kind < 0) return fail("word " + std::to_string(i) + " is no handler"), false;
    const size_t g = k == 0 ? 3 : 1 + (size_t)qt.data_words[tr[i] & 0xFFFFu];
    if (i + g > tr.size()) return fail("handler group at " + std::to_string(i) + " runs past the end"), false;
    if (blocks && i / 64 != (i + g - 1) / 64) return fail("handler group at " + std::to_string(i) + " straddles a block"), false;
    if (kinds) kinds->push_back(kind);
    if (kind == QK_END || kind == QK_END_V) {
      if (!blocks) {
        if (i + g != tr.size()) fail("END at " + std::to_string(i) + " is not the last word");
        return i + g == tr.size();
      }
      if (tr.size() % 64) return fail("the laid-out program is not whole blocks"), false;
      for (size_t j = i + 1; j < tr.size(); j++)
        if (kind_at(qt, 1, tr[j]) != QK_END) return fail("word " + std::to_string(j) + " behind END is not padding"), false;
      return true;
    }
    if (blocks && kind == QK_REFILL) i = (i / 64 + 1) * 64;
    else i += g;
  }
  return fail("no END"), false;
}

static void print_words(const char* tag, const std::vector<uint32_t>& w) {
  std::printf("%s", tag);
  for (uint32_t x : w) std::printf(" %x", x);
  std::printf("\n");
}

// One translation, made twice: the words and `extra` must repeat; the kind names go to stdout.
static void translation(const char* tag, const QsaTable& qt, const ModelLayout& ml, int k, bool models, const CompiledTape& x,
                        const std::vector<int>* gstage, bool g_bail) {
  std::vector<uint32_t> tr, ex, tr2, ex2;
  const bool ok = qsa_translate(qt, ml, k, models, x, &tr, &ex, nullptr, gstage, g_bail);
  const bool ok2 = qsa_translate(qt, ml, k, models, x, &tr2, &ex2, nullptr, gstage, g_bail);
  g_where += std::string(" ") + tag;
  if (ok != ok2 || (ok && (tr != tr2 || ex != ex2))) fail("a second translation differs");
  std::printf("%s %d", tag, ok ? 1 : 0);
  std::vector<int> before, after;
  if (ok) {
    walk(qt, k, tr, false, &before);
    for (int q : before) std::printf(" %s", kQsaKindNames[q]);
  }
  std::printf("\n");
  if (ok) print_words((std::string(tag) + "x").c_str(), ex);
  if (ok && k == 1) {
    qsa_window_layout(qt, tr);
    g_where += " laid out";
    if (walk(qt, 1, tr, true, &after)) {
      std::vector<int> kept;
      for (int q : after)
        if (q != QK_REFILL) kept.push_back(q);
      if (kept != before) fail("the layout changed the handlers");
    }
  }
  g_where.resize(g_where.rfind(std::string(" ") + tag));
}

// Everything the planners make of one batch of compiled tapes, as text.
static void planners(const std::string& name, const QsaTable& qt, const ModelLayout& ml, const std::vector<CompiledTape>& ct) {
  const int32_t n_tapes = (int32_t)ct.size();
  std::printf("batch %s\n", name.c_str());
  // the staging plan of the whole batch on G
  std::vector<int> gstage;
  std::vector<uint32_t> stage_rows;
  plan_stage(ml, count_pushes(ml, ct), nullptr, 0, 1.0, gstage, stage_rows);
  std::vector<std::vector<uint32_t>> fm(n_tapes);
  std::vector<std::vector<FcCmpH>> fq(n_tapes);
  std::vector<char> on_fc(n_tapes, 0), fneg(n_tapes, 0);
  for (int32_t t = 0; t < n_tapes; t++) {
    const CompiledTape& x = ct[t];
    g_where = name + " tape " + std::to_string(t);
    std::printf("tape %d supported %d L %d p_candidate %d\n", t, x.supported ? 1 : 0, x.L, p_candidate(x) ? 1 : 0);
    if (!x.supported || x.L != 8) continue;
    print_words("prog", x.prog);
    print_words("prog_g", x.prog_g);
    translation("P", qt, ml, 0, true, x, nullptr, false);
    translation("Gs", qt, ml, 1, false, x, nullptr, false);
    translation("G0", qt, ml, 1, true, x, nullptr, false);
    translation("G1", qt, ml, 1, true, x, nullptr, true);
    translation("G1s", qt, ml, 1, true, x, &gstage, true);
    {
      std::vector<uint32_t> pf, pf2;
      const bool ok = !x.prog_pf.empty() && qsa_translate_pf(qt, x, pf);
      g_where += " PF";
      std::printf("PF %d", ok ? 1 : 0);
      if (ok) {
        std::vector<int> kinds;
        walk(qt, 0, pf, false, &kinds);
        for (int q : kinds) std::printf(" %s", kQsaKindNames[q]);
        if (!qsa_translate_pf(qt, x, pf2) || pf2 != pf) fail("a second translation differs");
      }
      std::printf("\n");
    }
    bool ng = false;
    on_fc[t] = fc_match(ml, x, fm[t], fq[t], &ng, false) ? 1 : 0;
    fneg[t] = ng ? 1 : 0;
    std::printf("fc %d negated %d masks %zu compares %zu\n", (int)on_fc[t], (int)fneg[t], fm[t].size(), fq[t].size());
  }
  FcaPlan fap;
  fca_plan(ml, fm, fq, fneg, on_fc, [](size_t i) { return (uint32_t)i; },
           [&](size_t i) { return std::make_pair(ct[i].n_nodes, (uint32_t)ct[i].alg_ops); }, fap);
  std::printf("fca tapes %zu groups %zu atoms %zu segments %zu staged_rows %zu\n", fap.tape_out.size(), fap.groups.size(),
              fap.atoms.size(), fap.segs.size(), stage_rows.size());

}

// A program no tape of the compiler gives: bail points right behind variable pushes.  On G with
// the variables read from memory (PUSH_MEM) the first and the third find a load that nothing has
// waited for and must be dropped; the second follows the compare that read the load and stays.
// `extra` carries the second words of all three.
static CompiledTape bail_behind_push() {
  CompiledTape x;
  x.supported = true;
  x.L = 8;
  x.depth = 3;
  x.n_nodes = 8;
  x.alg_ops = 25;
  x.consts = {0x12345u, 0, 0, 0, 0, 0, 0, 0};
  x.prog = {gword(G_PUSH_VAR, 0, 8),   gword(G_BAIL, 0, 0), 300u,   // dropped: variable 8's load is in flight
            gword(G_PUSH_CONST, 1, 0), gword(G_EQ, 1, 256),
            gword(G_BAIL, 0, 0), 200u,                              // kept: the compare waited for the load
            gword(G_PUSH_VAR, 1, 9),   gword(G_PUSH_VAR, 2, 10),
            gword(G_BAIL, 0, 0), 100u,                              // dropped: two loads in flight
            gword(G_EQ, 2, 256),       gword(G_AND, 1, 0),          gword(G_END, 0, 0)};
  return x;
}

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: planner_check CORPUS\n"), 2;
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
  std::printf("kinds");
  for (int q = 0; q < QK_COUNT; q++) std::printf(" %s", kQsaKindNames[q]);
  std::printf("\n");
  const struct { const char* tag; const short* form; } forms[] = {
      {"andform", kQsaKindAndForm}, {"orform", kQsaKindOrForm}, {"notform", kQsaKindNot}, {"lform", kQsaKindLForm}};
  for (const auto& f : forms) {
    std::printf("%s", f.tag);
    for (int q = 0; q < QK_COUNT; q++) std::printf(" %d", (int)f.form[q]);
    std::printf("\n");
  }

  std::string word, name;
  while (in >> word) {
    int64_t n_vars, n_funcs, entry_words_n, n_tapes, n_nodes, n_consts;
    if (word != "batch" || !(in >> name >> n_vars >> n_funcs >> entry_words_n >> n_tapes >> n_nodes >> n_consts))
      return std::fprintf(stderr, "malformed batch header\n"), 2;
    ModelLayout ml;
    ml.entry_words_n = entry_words_n;
    uint32_t rows = 0;
    int32_t n_bool = 0;
    for (int64_t v = 0; v < n_vars; v++) {
      unsigned w;
      in >> w;
      ml.var_width.push_back((uint16_t)w);
      ml.var_off.push_back(rows);
      ml.var_nl.push_back(w == 0 ? 1 : (w + 31) / 32);
      ml.bmask_of_var.push_back(w == 0 ? n_bool++ : -1);
      rows += ml.var_nl.back();
    }
    for (int64_t f = 0; f < n_funcs; f++) {
      unsigned a, r, w0, w1;
      in >> a >> r >> w0 >> w1;
      ml.funcs.push_back(mq_func_desc{(uint16_t)a, (uint16_t)r, {(uint16_t)w0, (uint16_t)w1}});
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
    consts.resize(consts.size() + 1, 0);   // (an empty pool still has an address)
    mq_tape_batch tb{(int32_t)n_tapes, offsets.data(), nodes.data(), consts.data(), n_consts};

    CompileLimits lim;
    lim.g_depth = kQsaStackG;   // (as an upload compiles)
    std::vector<CompiledTape> ct;
    for (int32_t t = 0; t < n_tapes; t++) ct.push_back(compile_tape(&tb, t, lim));
    planners(name, qt, ml, ct);
  }
  {
    ModelLayout ml;   // eleven 256-bit variables
    for (uint32_t v = 0; v < 11; v++) {
      ml.var_width.push_back(256);
      ml.var_off.push_back(8 * v);
      ml.var_nl.push_back(8);
      ml.bmask_of_var.push_back(-1);
    }
    planners("handbuilt", qt, ml, {bail_behind_push()});
  }
  if (g_failures) std::fprintf(stderr, "%d checks failed\n", g_failures);
  return g_failures ? 1 : 0;
}
