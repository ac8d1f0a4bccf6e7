// qsa_translate.cpp — see qsa_translate.h.  Host only: no HIP header, no context.
#include "qsa_translate.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace mq {

bool QsaTable::build(const std::vector<uint32_t> (&offsets)[2], const uint32_t (&base_lo)[2]) {
  bool ok = true;
  for (int k = 0; k < 2; k++) {
    const int nh = k == 0 ? kQsaHandlersP : kQsaHandlersG;
    static_assert(kQsaStackP <= kQsaStack && kQsaStackG <= kQsaStack, "index holds both stacks");
    const QsaHandlerKey* keys = k == 0 ? kQsaHandlerKeysP : kQsaHandlerKeysG;
    for (int q = 0; q < QK_COUNT; q++)
      for (int d = 0; d < kQsaStack; d++)
        for (int v = 0; v <= kQsaSel; v++) index[k][q][d][v] = -1;
    for (int h = 0; h < nh; h++) index[k][keys[h].kind][keys[h].d < 0 ? 0 : keys[h].d][keys[h].v + 1] = h;
    if (offsets[k].size() != (size_t)nh) return false;
    off[k] = offsets[k];
    hbase_lo[k] = base_lo[k];
    // G's program words carry the handler word in 16 bits; P's entries carry absolute addresses,
    // so only this table bounds P's handler area (1 MB; the fused narrow handlers end past 256 KB)
    const uint32_t reach = k == 0 ? kQsaWordReachP : (1u << 16);
    kind_of[k].assign(reach, -1);
    for (int h = 0; h < nh; h++)
      if (hword(k, off[k][h]) < reach) kind_of[k][hword(k, off[k][h])] = (int16_t)keys[h].kind;
    uint32_t max_off = 0;
    for (int h = 0; h < nh; h++) {
      ok = ok && off[k][h] != 0xFFFFFFFFu && hword(k, off[k][h]) < reach &&
           (off[k][h] & ((k == 1 ? (1u << kQsaHandlerShiftG) : 4u) - 1)) == 0;
      max_off = std::max(max_off, off[k][h]);
    }
    // P program entries and G's decoded program window hold the low 32 bits of absolute handler
    // addresses: they must share the high half (the kernels keep it in s19)
    ok = ok && (uint64_t)hbase_lo[k] + max_off < (1ull << 32);
  }
  // G handler word index -> inline data words that follow it (generated: the window words the
  // handler body reads, gen_qsa.py handler_data_words)
  data_words.assign(1 << 16, 0);
  for (int h = 0; ok && h < kQsaHandlersG; h++)
    if (kQsaHandlerDataWordsG[h] > 0) data_words[hword(1, off[1][h]) & 0xFFFFu] = kQsaHandlerDataWordsG[h];
  for (int q = 0; q < QK_COUNT; q++) {
    const std::string n = kQsaKindNames[q];
    vm_drain[q] = n == "PUSH_MEMB" || n.rfind("MEQK", 0) == 0 || n.rfind("UF1", 0) == 0;
  }
  return ok;
}

// Count the handler kinds of one translated program (k = 0: P three-word entries; 1: G words,
// inline constant words skipped) into hist[QK_COUNT] and, if given, kind bigrams into pairs.
void qsa_count(const QsaTable& qt, int k, const std::vector<uint32_t>& tr, std::vector<int64_t>& hist,
               std::vector<int64_t>* pairs) {
  if (hist.size() != (size_t)QK_COUNT) hist.assign(QK_COUNT, 0);
  if (pairs && pairs->size() != (size_t)QK_COUNT * QK_COUNT) pairs->assign((size_t)QK_COUNT * QK_COUNT, 0);
  int prev = -1;
  for (size_t i = 0; i < tr.size();) {
    const uint32_t key = k == 0 ? ((tr[i] - qt.hbase_lo[0]) >> 2) & (kQsaWordReachP - 1) : tr[i] & 0xFFFFu;
    const int kind = qt.kind_of[k].empty() ? -1 : qt.kind_of[k][key];
    i += k == 0 ? 3 : 1;
    if (kind < 0) continue;
    hist[kind]++;
    if (pairs && prev >= 0 && kind != QK_REFILL) (*pairs)[(size_t)prev * QK_COUNT + kind]++;
    if (kind != QK_REFILL) prev = kind;
    if (k == 1) i += qt.data_words[key];
  }
}

// Translate a compiled stack program into QSA threaded code for kernel k (0 = P, 1 = G).
// models == false: structural check only (upload time: variable rows and function tables are
// not known yet, any variable / lookup is assumed expressible).  extra: the tape's derived
// constants (divisor reciprocals), appended after its own constants in the same order every
// time.  Returns false if any instruction is outside the interpreter's set (those tapes run on
// the HIP C++ kernel).  g_bail (the batch was uploaded under MQ_G_BAIL=1; verdict tapes only --
// never column programs, mode 3): for G a bail point becomes its BAIL word where no PUSH_MEM load
// can be outstanding, and the ops behind every bail point of the program follow the other
// derived constants in `extra`.
bool qsa_translate(const QsaTable& qt, const ModelLayout& ml, int k, bool models, const CompiledTape& x,
                   std::vector<uint32_t>* out_p, std::vector<uint32_t>* extra_p, const std::vector<int>* gpre,
                   const std::vector<int>* gstage, bool g_bail) {
  std::vector<uint32_t> dummy_out, dummy_extra;
  std::vector<uint32_t>& out = out_p ? *out_p : dummy_out;
  std::vector<uint32_t>& extra = extra_p ? *extra_p : dummy_extra;
  out.clear();
  extra.clear();
  const bool P = k == 0;
  if (x.L != 8 || qsa_depth(x, k) > (P ? kQsaStackP : kQsaStackG) || qsa_temps(x, k) > kQsaMaxTemps) return false;
  const std::vector<uint32_t>& xprog = qsa_prog(x, k);
  const size_t wpi = P ? 3 : 1;   // program words per interpreter instruction
  // every handler word emitted so far (position, key, immediate, inline data words): the
  // fusions below rewrite the last ones while nothing follows them
  struct Emit {
    size_t pos;
    int kind, d, v;
    uint32_t imm;
    size_t nd;
  };
  std::vector<Emit> log;
  auto ends_at = [&](const Emit& e) { return e.pos + wpi + e.nd; };
  auto drop_last = [&](size_t n) {   // forget the last n words (and their data)
    out.resize(log[log.size() - n].pos);
    log.resize(log.size() - n);
  };
  auto word = [&](int kind, int d, int v, uint32_t imm, bool imm32 = false) -> bool {
    if (d < 0 || d >= kQsaStack || v < -1 || v >= kQsaSel || (imm > 0xFFFFu && !(imm32 && P))) return false;
    const int h = qt.index[k][kind][d][v + 1];
    if (h < 0) return false;
    log.push_back(Emit{out.size(), kind, d, v, imm, 0});
    if (P) {   // entry: absolute handler address (low half), immediate, constant prefetch
      out.push_back(qt.hbase_lo[0] + qt.off[0][h]);
      out.push_back(imm);
      out.push_back(0);
    } else {
      out.push_back(hword(k, qt.off[k][h]) | (imm << 16));
    }
    return true;
  };
  // slot d holds a value of width W < 256: clear the bits above W
  auto mask = [&](int d, uint32_t W) -> bool {
    if (W >= 256) return true;
    const int n = (int)(W + 31) / 32;
    if (W % 32) return word(QK_MASKP, d, n - 1, W % 32);
    return word(QK_MASKZ, d, n - 1, 0);
  };
  auto lshr = [&](int d, uint32_t kbits, bool arith) -> bool {
    if (kbits == 0) return true;
    return word(arith ? QK_ASHRI : QK_LSHRI, d, (int)(kbits >> 5), kbits & 31);
  };
  auto shl = [&](int d, uint32_t kbits) -> bool {
    if (kbits == 0) return true;
    if (kbits & 31) return word(QK_SHLI, d, (int)(kbits >> 5), 32 - (kbits & 31));
    return word(QK_SHLW, d, (int)(kbits >> 5), 0);
  };
  // the constant pushed by the previous instruction (the right operand of a shift / division)
  auto const_value = [&](uint32_t off, uint32_t (&v)[8]) -> bool {
    if ((size_t)off + 8 > x.consts.size()) return false;
    for (int l = 0; l < 8; l++) v[l] = x.consts[off + l];
    return true;
  };
  // re-emit a word under another kind (same slot, selector, immediate and inline data)
  auto rekind = [&](int kind) -> bool {
    const Emit e = log.back();
    if (qt.index[k][kind][e.d][e.v + 1] < 0) return false;
    std::vector<uint32_t> data(out.begin() + (long)(e.pos + wpi), out.begin() + (long)ends_at(e));
    drop_last(1);
    if (!word(kind, e.d, e.v, e.imm)) return false;
    out.insert(out.end(), data.begin(), data.end());
    log.back().nd = data.size();
    return true;
  };
  // slot where the last word left a Bool result, or -1 (it is not a fusable Bool producer, or
  // something was emitted after it)
  auto last_bool_slot = [&]() -> int {
    if (log.empty() || out.size() != ends_at(log.back()) || kQsaKindBoolRes[log.back().kind] < 0) return -1;
    return kQsaKindBoolRes[log.back().kind] == 0 ? log.back().d : log.back().d - 1;
  };
  // AND / OR at slot d whose right operand the last word just produced: that word's fused form
  auto fuse_acc = [&](int d, bool is_and) -> bool {
    if (last_bool_slot() != d) return false;
    const int fk = is_and ? kQsaKindAndForm[log.back().kind] : kQsaKindOrForm[log.back().kind];
    return fk >= 0 && rekind(fk);
  };
  // NOT of a compare the last word just made: the complementary compare
  auto fuse_not = [&](int d) -> bool {
    if (last_bool_slot() != d || kQsaKindNot[log.back().kind] < 0) return false;
    return rekind(kQsaKindNot[log.back().kind]);
  };
  // G: a constant push as the operand of a compare -> the compare-with-inline-constant handler.
  // (cls, data words) of the constant pushed by e (PUSH_CONSTI / PUSH_CONSTW), or cls -1
  auto const_of = [&](const Emit& e, std::vector<uint32_t>& words) -> int {
    words.clear();
    if (e.kind == QK_PUSH_CONSTI) return 0;
    if (e.kind != QK_PUSH_CONSTW) return -1;
    const size_t n = e.nd;
    words.assign(out.begin() + (long)(e.pos + 1), out.begin() + (long)(e.pos + 1 + n));
    const int cls = n <= (size_t)kQsaKClassWords[1] ? 1 : 2;
    words.resize((size_t)kQsaKClassWords[cls], 0);
    return cls;
  };
  auto emit_k = [&](int kind, int x, int sel, uint32_t imm, const std::vector<uint32_t>& words) -> bool {
    if (!word(kind, x, sel, imm)) return false;
    out.insert(out.end(), words.begin(), words.end());
    log.back().nd = words.size();
    return true;
  };
  // compare `kind` at slot d (operands S(d-1), S(d)); kk = its constant form, mk = the constant
  // form of the mirrored compare (c OP x == x MIRROR(OP) c)
  auto fuse_const = [&](int d, int kk, int mk) -> bool {
    if (P || log.empty() || d < 1) return false;
    std::vector<uint32_t> words;
    const Emit e1 = log.back();
    if (out.size() != ends_at(e1)) return false;
    // constant on the right: S(d-1) OP c
    if (e1.d == d) {
      const int cls = const_of(e1, words);
      if (cls >= 0 && qt.index[k][kk][d - 1][cls + 1] >= 0) {
        const uint32_t imm = e1.imm;
        drop_last(1);
        return emit_k(kk, d - 1, cls, cls == 0 ? imm : 0, words);
      }
    }
    // constant on the left, value pushed right after it: the value moves down one slot
    if (log.size() >= 2 && e1.d == d && e1.nd == 0 &&
        (e1.kind == QK_PUSH_MEM || e1.kind == QK_PUSH_MEMS || e1.kind == QK_PUSH_TMP || e1.kind == QK_PUSH_VAR)) {
      const Emit e0 = log[log.size() - 2];
      const int cls = e0.d == d - 1 && ends_at(e0) == e1.pos ? const_of(e0, words) : -1;
      if (cls >= 0 && qt.index[k][mk][d - 1][cls + 1] >= 0 && qt.index[k][e1.kind][d - 1][e1.v + 1] >= 0) {
        const uint32_t imm = e0.imm;
        drop_last(2);
        return word(e1.kind, d - 1, e1.v, e1.imm) && emit_k(mk, d - 1, cls, cls == 0 ? imm : 0, words);
      }
    }
    return false;
  };
  // G: consecutive "B(d - 1) &= packed mask" words (PUSH_PKB_A at slot d) as one PKBN_A word
  // with up to four masks: their scalar loads share one wait
  // ... and a PUSH_PKB at slot d - 1 followed by such words as one PKBP word at d - 1 (their AND
  // pushed); up to six masks a word
  auto merge_pkb = [&](int d) {
    if (log.size() < 2) return;
    const Emit e1 = log.back();
    if (e1.kind != QK_PUSH_PKB_A || e1.d != d || out.size() != ends_at(e1)) return;
    const Emit e0 = log[log.size() - 2];
    if (ends_at(e0) != e1.pos) return;
    int n0, kind, x;   // masks after the first one in e0; merged kind and slot
    if (e0.d == d && e0.kind == QK_PUSH_PKB_A) n0 = 0, kind = QK_PKBN_A, x = d;
    else if (e0.d == d && e0.kind == QK_PKBN_A) n0 = e0.v, kind = QK_PKBN_A, x = d;
    else if (e0.d == d - 1 && e0.kind == QK_PUSH_PKB) n0 = 0, kind = QK_PKBP, x = d - 1;
    else if (e0.d == d - 1 && e0.kind == QK_PKBP) n0 = e0.v, kind = QK_PKBP, x = d - 1;
    else return;
    if (n0 + 1 > 5 || qt.index[k][kind][x][n0 + 2] < 0) return;
    std::vector<uint32_t> data(out.begin() + (long)(e0.pos + 1), out.begin() + (long)ends_at(e0));
    data.push_back(e1.imm);
    const uint32_t imm0 = e0.imm;
    drop_last(2);
    emit_k(kind, x, n0 + 1, imm0, data);
  };
  // G: "PUSH_MEM / PUSH_MEMS x (n limbs); EQK_A x" (a model variable compared with an inline
  // constant, AND-ed into the conjunction) as one M/SEQK{2,8}_A word: row / slot in the
  // immediate, the constant in 2 or 8 inline data words (a 16-bit immediate constant travels
  // as two)
  // (and "PUSH_MEMS x; ULTK_A / UGTK_A x" as one S{ULT,UGT}K{2,8}_A word, same layout)
  auto merge_memk = [&]() {
    if (log.size() < 2) return;
    const Emit e1 = log.back();
    if ((e1.kind != QK_EQK_A && e1.kind != QK_ULTK_A && e1.kind != QK_UGTK_A) || out.size() != ends_at(e1)) return;
    const Emit e0 = log[log.size() - 2];
    if (ends_at(e0) != e1.pos || e0.d != e1.d || e0.nd != 0 || e0.v < 0) return;
    const bool wide = e1.v == 2;
    int fk;
    if (e1.kind == QK_ULTK_A) {
      if (e0.kind != QK_PUSH_MEMS) return;
      fk = wide ? QK_SULTK8_A : QK_SULTK2_A;
    } else if (e1.kind == QK_UGTK_A) {
      if (e0.kind != QK_PUSH_MEMS) return;
      fk = wide ? QK_SUGTK8_A : QK_SUGTK2_A;
    } else if (e0.kind == QK_PUSH_MEM) fk = wide ? QK_MEQK8_A : QK_MEQK2_A;
    else if (e0.kind == QK_PUSH_MEMS) fk = wide ? QK_SEQK8_A : QK_SEQK2_A;
    else return;
    if (qt.index[k][fk][e1.d][e0.v + 1] < 0) return;
    std::vector<uint32_t> data;
    if (e1.v == 0) data = {e1.imm, 0u};
    else data.assign(out.begin() + (long)(e1.pos + 1), out.begin() + (long)ends_at(e1));
    const int x = e1.d, nsel = e0.v;
    const uint32_t imm0 = e0.imm;
    drop_last(2);
    emit_k(fk, x, nsel, imm0, data);
  };
  // G: "PUSH_MEMS x (n limbs); SLTK / SGTK x" as one S{SLT,SGT}K{2,8} word (layout as merge_memk's)
  auto merge_mems_k = [&]() {
    if (P || log.size() < 2) return;
    const Emit e1 = log.back();
    if ((e1.kind != QK_SLTK && e1.kind != QK_SGTK) || out.size() != ends_at(e1)) return;
    const Emit e0 = log[log.size() - 2];
    if (e0.kind != QK_PUSH_MEMS || ends_at(e0) != e1.pos || e0.d != e1.d || e0.nd != 0 || e0.v < 0) return;
    const bool wide = e1.v == 2;
    const int fk = e1.kind == QK_SLTK ? (wide ? QK_SSLTK8 : QK_SSLTK2) : (wide ? QK_SSGTK8 : QK_SSGTK2);
    if (qt.index[k][fk][e1.d][e0.v + 1] < 0) return;
    std::vector<uint32_t> data;
    if (e1.v == 0) data = {e1.imm, 0u};
    else data.assign(out.begin() + (long)(e1.pos + 1), out.begin() + (long)ends_at(e1));
    const int x = e1.d, nsel = e0.v;
    const uint32_t imm0 = e0.imm;
    drop_last(2);
    emit_k(fk, x, nsel, imm0, data);
  };
  // G: may a PUSH_MEM's vector loads be outstanding after the words emitted so far?  The final
  // pass's rule, read backwards: a PUSH_MEM not yet followed by a stack reader (either wait form
  // of one drains, or finds nothing to drain) or by a handler that waits for vector memory itself
  auto push_mem_pending = [&]() -> bool {
    for (size_t i = log.size(); i-- > 0;) {
      if (log[i].kind == QK_PUSH_MEM) return true;
      if (kQsaKindLForm[log[i].kind] >= 0 || qt.vm_drain[log[i].kind]) return false;
    }
    return false;
  };
  // G under g_bail: the ops behind every bail point of the program, kept or dropped, in program
  // order -- appended to `extra` after the division constants, whose offsets they leave alone (P
  // translates the unspilled program, with its own bail points, against the same pool)
  std::vector<uint32_t> bail_ops;
  uint32_t prev_op = G_END, prev_d = 0, prev_imm = 0;
  size_t prev_out = 0;
  int prev_pre = -1;   // preload slot of the variable the previous instruction pushed
  // preload slot of variable v in this kernel, or -1 (P: v itself; G: the batch's choice)
  auto pre_slot = [&](uint32_t v) -> int {
    if (P) return v < (uint32_t)kQsaVars ? (int)v : -1;
    if (!models || !gpre || v >= gpre->size()) return -1;
    return (*gpre)[v];
  };
  // a binary op at slot d whose right operand was just pushed from a preloaded variable runs
  // as the fused handler kindv(d, slot) (the push word is dropped)
  // (P) likewise a right operand just pushed from the constants, for the kinds with a kindc
  // handler (operand read from SGPRs)
  auto binop = [&](int d, int kind, int kindv, int kindc = -1, int kindk = -1, int kindkm = -1) -> bool {
    // G: EQ of a constant (left) and a preloaded variable (right) -> EQVK, no stack traffic
    if (!P && kind == QK_EQ && prev_op == G_PUSH_VAR && prev_pre >= 0 && (int)prev_d == d && log.size() >= 2 &&
        out.size() == prev_out + wpi && log.back().pos == prev_out) {
      const Emit e0 = log[log.size() - 2];
      std::vector<uint32_t> words;
      int cls = e0.d == d - 1 && ends_at(e0) == prev_out ? const_of(e0, words) : -1;
      if (cls == 0) {   // the 16-bit immediate travels as a two-word constant here
        words.assign((size_t)kQsaKClassWords[1], 0);
        words[0] = e0.imm;
        cls = 1;
      }
      const int sel = 2 * prev_pre + (cls - 1);
      if (cls >= 1 && sel < kQsaSel && qt.index[k][QK_EQVK][d - 1][sel + 1] >= 0) {
        drop_last(2);
        return emit_k(QK_EQVK, d - 1, sel, 0, words);
      }
    }
    if (kindk >= 0 && fuse_const(d, kindk, kindkm)) return true;
    if (prev_op == G_PUSH_VAR && prev_pre >= 0 && (int)prev_d == d && out.size() == prev_out + wpi &&
        qt.index[k][kindv][d][prev_pre + 1] >= 0) {
      drop_last(1);
      // (P) the left operand is a leaf pushed right before at slot d - 1: both leaves in one
      // handler at d - 1 (gen_qsa.py kindVV / MULVV / kindCV, the right variable through M0)
      int kvv = -1, kcv = -1;
      bool vv_by_v1 = true;
      switch (kindv) {
        case QK_ADDV: kvv = QK_ADDVV; kcv = QK_ADDCV; break;
        case QK_SUBV: kvv = QK_SUBVV; kcv = QK_SUBCV; break;
        case QK_BANDV: kvv = QK_BANDVV; kcv = QK_BANDCV; break;
        case QK_BORV: kvv = QK_BORVV; kcv = QK_BORCV; break;
        case QK_BXORV: kvv = QK_BXORVV; kcv = QK_BXORCV; break;
        case QK_MULV: kvv = QK_MULVV; kcv = QK_MULCV; vv_by_v1 = false; break;
        default: break;
      }
      if (P && kvv >= 0 && d >= 1 && !log.empty() && out.size() == ends_at(log.back()) && log.back().d == d - 1) {
        const Emit e0 = log.back();
        const uint32_t v2 = 8u * (uint32_t)prev_pre;
        if (e0.kind == QK_PUSH_VAR && e0.v >= 0 && qt.index[k][kvv][d - 1][vv_by_v1 ? e0.v + 1 : 0] >= 0) {
          drop_last(1);
          return vv_by_v1 ? word(kvv, d - 1, e0.v, v2) : word(kvv, d - 1, -1, 8u * (uint32_t)e0.v | v2 << 16, true);
        }
        if (e0.kind == QK_PUSH_CONST && qt.index[k][kcv][d - 1][0] >= 0) {
          drop_last(1);
          return word(kcv, d - 1, -1, e0.imm | v2 << 16, true);
        }
      }
      return word(kindv, d, prev_pre, 0);
    }
    if (kindc >= 0 && P && prev_op == G_PUSH_CONST && (int)prev_d == d && out.size() == prev_out + wpi &&
        qt.index[k][kindc][d][0] >= 0) {
      drop_last(1);
      return word(kindc, d, -1, prev_imm);
    }
    return word(kind, d, -1, 0);
  };
  for (size_t pc = 0; pc < xprog.size(); pc++) {
    const uint32_t w = xprog[pc];
    const uint32_t op = w & 0xFFu, imm = w >> 12;
    const int d = (int)((w >> 8) & 0xFu);
    uint32_t imm2 = 0;
    if (has_imm2(op)) {
      if (++pc >= xprog.size()) return false;
      imm2 = xprog[pc];
    }
    // a bail point is P's and, under MQ_G_BAIL=1 (g_bail), G's on verdict tapes.  G takes it
    // only where no PUSH_MEM load can be outstanding (a load landing in a stack register after
    // the next tape has started would corrupt that tape): at a spine point every push has been
    // consumed by the compare that made B(0), which the emitted words must confirm.  Dropped, the
    // word leaves the fusions' view of the previous instruction untouched.  (The ops behind it
    // are recorded either way: every translation of a program lays its constants out the same.)
    if (op == G_BAIL && !P) {
      if (!g_bail) continue;
      bail_ops.push_back(imm2);
      if (d != 0 || bail_ops.size() > 0xFFFFu || push_mem_pending()) continue;
    }
    const size_t out_before = out.size();
    const bool after_const = prev_op == G_PUSH_CONST && (int)prev_d == d;
    int pushed_pre = -1;
    bool ok;
    switch (op) {
      case G_END: ok = word(QK_END, 0, -1, 0); break;
      // P: an entry without a constant (an ordinary non-PF_ entry to the constant prefetch
      // pass); its 32-bit immediate is the ops the rest of the program would cost
      // G: the ops do not fit the 16-bit immediate: it is the index into bail_ops here and
      // becomes the word's offset in the tape's constants below (the handler loads it when it
      // leaves the tape, and only then)
      case G_BAIL: ok = d == 0 && (P ? word(QK_BAIL, 0, -1, imm2, true) : word(QK_BAIL, 0, -1, (uint32_t)bail_ops.size() - 1)); break;
      case G_PUSH_VAR:
      case G_PUSH_VAR_B: {
        const bool b = op == G_PUSH_VAR_B;
        const int ps = pre_slot(imm);
        if (P) {
          // preloaded variables only (var < 8, at most 256 bits)
          ok = ps >= 0 && (!models || (imm < ml.var_nl.size() && ml.var_nl[imm] <= 8)) &&
               word(b ? QK_PUSH_VARB : QK_PUSH_VAR, d, ps, 0);
          pushed_pre = ps;
        } else if (ps >= 0) {
          ok = word(b ? QK_PUSH_VARB : QK_PUSH_VAR, d, ps, 0);
          pushed_pre = ps;
        } else if (!models) {
          ok = word(b ? QK_PUSH_MEMB : QK_PUSH_MEM, d, b ? -1 : 7, 0);
        } else if (b && imm < ml.bmask_of_var.size() && ml.bmask_of_var[imm] >= 0) {
          // the tile's lane mask, one scalar load (qs_pack_bool)
          ok = word(QK_PUSH_PKB, d, -1, (uint32_t)ml.bmask_of_var[imm]);
        } else if (gstage && imm < gstage->size() && (*gstage)[imm] >= 0 && ml.var_nl[imm] <= 8) {
          // a row staged in LDS by the workgroup (gen_qsa.py stage_rows)
          ok = word(b ? QK_PUSH_MEMSB : QK_PUSH_MEMS, d, b ? -1 : (int)ml.var_nl[imm] - 1, (uint32_t)(*gstage)[imm]);
        } else {
          ok = imm < ml.var_off.size() && ml.var_nl[imm] <= 8 && ml.var_off[imm] <= 0xFFFFu &&
               word(b ? QK_PUSH_MEMB : QK_PUSH_MEM, d, b ? -1 : (int)ml.var_nl[imm] - 1, ml.var_off[imm]);
        }
        break;
      }
      case G_PUSH_CONST: {
        if (P) {
          ok = word(QK_PUSH_CONST, d, -1, imm);
          break;
        }
        // G: the constant travels inline in the program stream (no scalar load)
        uint32_t cv[8];
        ok = const_value(imm, cv);
        if (!ok) break;
        int n = 8;
        while (n > 1 && cv[n - 1] == 0) n--;
        if (n == 1 && cv[0] <= 0xFFFFu) {
          ok = word(QK_PUSH_CONSTI, d, -1, cv[0]);
        } else {
          ok = word(QK_PUSH_CONSTW, d, n - 1, 0);
          for (int l = 0; ok && l < n; l++) out.push_back(cv[l]);
          if (ok) log.back().nd = (size_t)n;
        }
        break;
      }
      case G_PUSH_TMP: ok = word(QK_PUSH_TMP, d, -1, imm); break;
      case G_PUSH_TMP_B: ok = word(QK_PUSH_TMP_BOOL, d, -1, imm); break;
      case G_STORE_TMP: ok = d == 0 && word(QK_STORE_TMP, 0, -1, imm); break;
      case G_STORE_TMP_B: ok = d == 0 && word(QK_STORE_TMP_BOOL, 0, -1, imm); break;
      case G_PUSH_BOOL: ok = word(QK_PUSH_BOOL, d, -1, imm); break;
      case G_NOT: ok = fuse_not(d) || word(QK_NOT, d, -1, 0); break;
      case G_AND:
        ok = fuse_acc(d, true) || word(QK_AND, d, -1, 0);
        if (ok && !P) merge_pkb(d);
        if (ok && !P) merge_memk();
        break;
      case G_OR: ok = fuse_acc(d, false) || word(QK_OR, d, -1, 0); break;
      case G_XOR: ok = word(QK_XOR, d, -1, 0); break;
      case G_IFF: ok = word(QK_IFF, d, -1, 0); break;
      case G_IMPLIES: ok = word(QK_IMPLIES, d, -1, 0); break;
      case G_BITE: ok = word(QK_BITE, d, -1, 0); break;
      case G_BITE_EF: ok = word(QK_BITE_EF, d, -1, 0); break;
      // unsigned predicates / bitwise / ite are exact on canonical values of any width <= 256
      case G_EQ: ok = imm >= 1 && binop(d, QK_EQ, QK_EQV, QK_EQC, QK_EQK, QK_EQK); break;
      case G_ULT: ok = imm >= 1 && binop(d, QK_ULT, QK_ULTV, QK_ULTC, QK_ULTK, QK_UGTK); break;
      case G_ULE: ok = imm >= 1 && binop(d, QK_ULE, QK_ULEV, QK_ULEC, QK_ULEK, QK_UGEK); break;
      case G_UGT: ok = imm >= 1 && binop(d, QK_UGT, QK_UGTV, QK_UGTC, QK_UGTK, QK_ULTK); break;
      case G_UGE: ok = imm >= 1 && binop(d, QK_UGE, QK_UGEV, QK_UGEC, QK_UGEK, QK_ULEK); break;
      case G_BAND: ok = binop(d, QK_BAND, QK_BANDV, QK_BANDC); break;
      case G_BOR: ok = binop(d, QK_BOR, QK_BORV, QK_BORC); break;
      case G_BXOR: ok = binop(d, QK_BXOR, QK_BXORV, QK_BXORC); break;
      case G_ITE: {
        // G: ite(c, x, 0) with the zero pushed last -> ITEZ at the then-slot (the push dropped)
        const Emit* e = log.empty() ? nullptr : &log.back();
        if (!P && d >= 2 && e && e->kind == QK_PUSH_CONSTI && e->imm == 0 && e->d == d && out.size() == ends_at(*e) &&
            qt.index[k][QK_ITEZ][d - 1][0] >= 0) {
          drop_last(1);
          // "SS{LT,GT}K x; PUSH_MEM x + 1": the load goes first, so it is in flight while the
          // compare reads LDS (the compare touches slot x, T and B(x) only)
          if (log.size() >= 2) {
            const Emit ep = log.back(), ec = log[log.size() - 2];
            const bool cmp = ec.kind == QK_SSLTK2 || ec.kind == QK_SSGTK2 || ec.kind == QK_SSLTK8 || ec.kind == QK_SSGTK8;
            if (cmp && ep.kind == QK_PUSH_MEM && ep.nd == 0 && ep.d == d - 1 && ec.d == d - 2 &&
                ends_at(ec) == ep.pos && out.size() == ends_at(ep)) {
              std::vector<uint32_t> data(out.begin() + (long)(ec.pos + 1), out.begin() + (long)ends_at(ec));
              drop_last(2);
              ok = word(ep.kind, ep.d, ep.v, ep.imm) && emit_k(ec.kind, ec.d, ec.v, ec.imm, data);
              if (!ok) break;
            }
          }
          // a staged then-value pushed right before: ITEZS reads the row itself
          const Emit ev = log.empty() ? Emit{} : log.back();
          if (!log.empty() && ev.kind == QK_PUSH_MEMS && ev.nd == 0 && ev.d == d - 1 && ev.v >= 0 && out.size() == ends_at(ev) &&
              qt.index[k][QK_ITEZS][d - 1][ev.v + 1] >= 0) {
            const int nsel = ev.v;
            const uint32_t row = ev.imm;
            drop_last(1);
            ok = word(QK_ITEZS, d - 1, nsel, row);
            break;
          }
          ok = word(QK_ITEZ, d - 1, -1, 0);
        } else ok = word(QK_ITE, d, -1, 0);
        break;
      }
      case G_ITE_EF: ok = word(QK_ITE_EF, d, -1, 0); break;
      // signed predicates: at 256 bits the handler flips bit 255; below, flip bit W-1 of both
      // operands (FLIP2) and compare unsigned
      case G_SLT: case G_SLE: case G_SGT: case G_SGE: {
        const int su = op == G_SLT ? QK_SLT : op == G_SLE ? QK_SLE : op == G_SGT ? QK_SGT : QK_SGE;
        const int uu = op == G_SLT ? QK_ULT : op == G_SLE ? QK_ULE : op == G_SGT ? QK_UGT : QK_UGE;
        if (imm == 256 && (op == G_SLT || op == G_SGT) &&
            fuse_const(d, op == G_SLT ? QK_SLTK : QK_SGTK, op == G_SLT ? QK_SGTK : QK_SLTK)) {
          // G: a compare with a constant operand; a staged variable pushed right before it is
          // read by the compare itself (S{SLT,SGT}K{2,8})
          merge_mems_k();
          ok = true;
        } else if (imm == 256) ok = word(su, d, -1, 0);
        else ok = imm >= 1 && imm < 256 && word(QK_FLIP2, d, (int)((imm - 1) >> 5), (imm - 1) & 31) && word(uu, d, -1, 0);
        break;
      }
      // wrapping arithmetic: 256-bit handlers, results below 256 bits re-masked
      case G_ADD: ok = imm <= 256 && binop(d, QK_ADD, QK_ADDV, QK_ADDC) && mask(d - 1, imm); break;
      case G_SUB: ok = imm <= 256 && binop(d, QK_SUB, QK_SUBV, QK_SUBC) && mask(d - 1, imm); break;
      case G_MUL: ok = imm <= 256 && binop(d, QK_MUL, QK_MULV, QK_MULC) && mask(d - 1, imm); break;
      case G_NEG: ok = imm <= 256 && word(QK_NEG, d, -1, 0) && mask(d, imm); break;
      case G_BNOT: ok = imm <= 256 && word(QK_BNOT, d, -1, 0) && mask(d, imm); break;
      // shifts by a constant amount (the previous instruction pushed it): in place on slot d-1
      case G_SHL: case G_LSHR: case G_ASHR: {
        uint32_t cv[8];
        if (!after_const) {   // by a variable amount: G's SHLV / LSHRV / ASHRV (ASHR at 256 bits);
          // the immediate is the width W: the handler replaces results of amounts >= W by the fill
          ok = d >= 1 && imm >= 1 && imm <= 256 && (op != G_ASHR || imm == 256) &&
               word(op == G_SHL ? QK_SHLV : op == G_LSHR ? QK_LSHRV : QK_ASHRV, d - 1, -1, imm) &&
               (op != G_SHL || mask(d - 1, imm));
          break;
        }
        ok = after_const && d >= 1 && imm >= 1 && imm <= 256 && const_value(prev_imm, cv);
        if (!ok) break;
        if (log.empty() || log.back().pos != prev_out) return false;
        drop_last(1);  // drop the amount push
        bool big = false;
        for (int l = 1; l < 8; l++) big = big || cv[l] != 0;
        const uint32_t kb = big || cv[0] >= imm ? imm : cv[0];  // >= width: everything shifted out
        if (op == G_ASHR) {
          ok = imm == 256 && lshr(d - 1, std::min<uint32_t>(kb, 255), true);
        } else if (kb >= imm) {
          ok = word(QK_MASKP, d - 1, 0, 0);  // zero
        } else if (op == G_LSHR) {
          ok = lshr(d - 1, kb, false);
        } else {
          ok = shl(d - 1, kb) && mask(d - 1, imm);
        }
        break;
      }
      // division by a constant divisor (the previous instruction pushed it), in place on d-1
      case G_UDIV: case G_UREM: case G_SDIV: case G_SREM: case G_SMOD: {
        uint32_t cv[8];
        if (!after_const) {
          // by a variable divisor: G's UDIVV / UREMV (both slots; the quotient of x / 0 is all
          // ones, masked back to the width) and, at 256 bits, SDIVV / SREMV / SMODV
          int kind = op == G_UDIV ? QK_UDIVV : op == G_UREM ? QK_UREMV : op == G_SDIV ? QK_SDIVV
                   : op == G_SREM ? QK_SREMV : QK_SMODV;
          const bool sgn = op == G_SDIV || op == G_SREM || op == G_SMOD;
          ok = d >= 1 && imm >= 1 && imm <= 256 && (!sgn || imm == 256) && word(kind, d - 1, -1, 0) &&
               (op != G_UDIV || mask(d - 1, imm));
          break;
        }
        if (op == G_UDIV || op == G_UREM) {
          // unsigned by a constant that is not a non-zero 32-bit value: UDIVV / UREMV on it
          bool small = const_value(prev_imm, cv) && cv[0] != 0;
          for (int l = 1; small && l < 8; l++) small = cv[l] == 0;
          if (!small) {
            ok = d >= 1 && imm >= 1 && imm <= 256 && word(op == G_UDIV ? QK_UDIVV : QK_UREMV, d - 1, -1, 0) &&
                 (op == G_UREM || mask(d - 1, imm));
            break;
          }
        }
        ok = after_const && d >= 1 && imm >= 1 && imm <= 256 && const_value(prev_imm, cv);
        if (!ok) break;
        const bool sgn = op == G_SDIV || op == G_SREM || op == G_SMOD;
        bool neg = false;
        if (sgn) {
          if (imm != 256) { ok = false; break; }
          neg = (cv[7] >> 31) != 0;
          if (neg) {  // |c| = -c
            uint64_t br = 1;
            for (int l = 0; l < 8; l++) {
              const uint64_t t = (uint64_t)(uint32_t)~cv[l] + br;
              cv[l] = (uint32_t)t;
              br = t >> 32;
            }
          }
        }
        bool hi = false;
        for (int l = 1; l < 8; l++) hi = hi || cv[l] != 0;
        if (sgn && (hi || cv[0] == 0)) {
          // a signed divisor of 0 or of magnitude >= 2^32: SDIVV / SREMV / SMODV on the pushed
          // constant, as the unsigned case routes such divisors to UDIVV / UREMV (G only)
          ok = word(op == G_SDIV ? QK_SDIVV : op == G_SREM ? QK_SREMV : QK_SMODV, d - 1, -1, 0);
          break;
        }
        if (log.empty() || log.back().pos != prev_out) return false;
        drop_last(1);  // drop the divisor push
        if (!sgn && !hi && cv[0] != 0 && (cv[0] & (cv[0] - 1)) == 0) {
          // unsigned power of two: shift / mask
          const uint32_t kb = (uint32_t)__builtin_ctz(cv[0]);
          ok = op == G_UDIV ? lshr(d - 1, kb, false)
                            : (kb == 0 ? word(QK_MASKP, d - 1, 0, 0) : mask(d - 1, kb));
          break;
        }
        if (hi || cv[0] == 0) { ok = false; break; }
        const uint32_t cabs = cv[0];
        const uint32_t sh = (uint32_t)__builtin_clz(cabs);
        const uint32_t dn = cabs << sh;
        const uint64_t inv = ~0ull / dn - (1ull << 32);
        const uint32_t off = (uint32_t)(x.consts.size() + extra.size());
        extra.push_back(dn);
        extra.push_back((uint32_t)inv);
        extra.push_back(sh);
        extra.push_back(cabs);
        int kind;
        switch (op) {
          case G_UDIV: kind = QK_UDIVC; break;
          case G_UREM: kind = QK_UREMC; break;
          case G_SREM: kind = QK_SREMC; break;
          case G_SMOD: kind = neg ? QK_SMODCN : QK_SMODCP; break;
          default: kind = neg ? QK_SDIVCN : QK_SDIVCP; break;
        }
        ok = word(kind, d - 1, -1, off);
        break;
      }
      case G_EXTRACT:  // imm = lo, imm2 = result width
        ok = imm < 256 && imm2 >= 1 && imm2 <= 256 && lshr(d, imm, false) && mask(d, imm2);
        break;
      case G_CONCAT:  // imm = width of the low operand (slot d), imm2 = result width
        ok = imm >= 1 && imm < 256 && imm2 <= 256;
        if (ok && !P && (imm & 31) && qt.index[k][QK_SHLOR][d][(imm >> 5) + 1] >= 0)
          ok = word(QK_SHLOR, d, (int)(imm >> 5), 32 - (imm & 31));   // G: shift and OR in one
        else ok = ok && shl(d - 1, imm) && word(QK_BOR, d, -1, 0);
        break;
      case G_SEXT: {  // imm = source width, imm2 = result width
        ok = imm >= 1 && imm <= 256 && imm2 <= 256;
        if (!ok) break;
        const int p = (int)((imm - 1) >> 5);
        const uint32_t nb = ((imm - 1) & 31) + 1;
        if (nb < 32) ok = word(QK_SEXTB, d, p, nb);
        else if (p < 7) ok = word(QK_SEXTA, d, p, 0);
        ok = ok && mask(d, imm2);
        break;
      }
      case G_UF1: {  // imm = function id, imm2 = result width (0 = Bool)
        // (G scans the entries with 32-bit byte offsets)
        ok = !P && imm2 <= 256 && (uint64_t)(ml.entry_words_n + (int64_t)kEntryPadWords) * 4 < (1ull << 32);
        if (ok && models) {
          // a function absent from the model batch evaluates to 0 (as in the C++ kernel)
          ok = imm >= ml.funcs.size() || (ml.funcs[imm].arity == 1 && ml.funcs[imm].arg_width[0] <= 256 &&
                                            ml.funcs[imm].result_width <= 256);
        }
        if (!ok) break;
        if (imm2 == 0) ok = word(QK_UF1B, d, -1, imm);
        else ok = word(QK_UF1, d, -1, imm) && mask(d, imm2);
        break;
      }
      default: ok = false;
    }
    if (!ok) {
      // MQ_QSA_DEBUG=1: name the stack-program instruction a translation stops at (diagnostic)
      static const bool dbg = std::getenv("MQ_QSA_DEBUG") != nullptr;
      if (dbg) std::fprintf(stderr, "qsa_translate(%s): op %u at slot %d imm %u not translated\n", P ? "P" : "G", op, d, imm);
      return false;
    }
    prev_op = op;
    prev_d = (uint32_t)d;
    prev_imm = imm;
    prev_out = out_before;
    prev_pre = op == G_PUSH_VAR ? pushed_pre : -1;
  }
  static const bool no_lwait = std::getenv("MQ_NO_LWAIT") != nullptr;   // (diagnostic A/B)
  if (!P) {
    // final pass: a stack reader waits for the vector loads of a PUSH_MEM only when one may be
    // outstanding; otherwise its "_L" variant waits for LDS / scalar loads alone, and the
    // prefetch of the next program window (gen_qsa.py load_window) stays in flight
    // (MQ_NO_LWAIT: no _L variants; END_V is needed either way)
    bool pending = false;
    std::vector<const Emit*> unsafe_bails;
    for (const Emit& e : log) {
      if (e.kind == QK_PUSH_MEM) {
        pending = true;
        continue;
      }
      if (e.kind == QK_BAIL) {
        // this pass is the authority on loads in flight: a bail word it finds behind an
        // outstanding PUSH_MEM goes (push_mem_pending kept it out when it was emitted)
        if (pending) unsafe_bails.push_back(&e);
        continue;
      }
      if (e.kind == QK_END) {
        // the value a column stores may still be a load in flight: END_V waits for it (the
        // tape end's column store waits for LDS / scalar loads only)
        const int h = qt.index[k][QK_END_V][0][0];
        if (pending && h >= 0) out[e.pos] = hword(k, qt.off[k][h]);
        continue;
      }
      const int lk = kQsaKindLForm[e.kind];
      if (lk >= 0) {
        const int h = qt.index[k][lk][e.d][e.v + 1];
        if (!pending && h >= 0 && !no_lwait) out[e.pos] = hword(k, qt.off[k][h]) | (e.imm << 16);
        pending = false;   // (the VMWAIT form drained every load)
        continue;
      }
      if (qt.vm_drain[e.kind]) pending = false;
    }
    // the kept bail words name their ops by offset in the tape's constants; one past the
    // immediate's reach goes too
    const size_t bail_base = x.consts.size() + extra.size();
    for (const Emit& e : log) {
      if (e.kind != QK_BAIL) continue;
      const size_t off = bail_base + e.imm;
      const bool gone = std::find(unsafe_bails.begin(), unsafe_bails.end(), &e) != unsafe_bails.end();
      if (off > 0xFFFFu && !gone) unsafe_bails.push_back(&e);
      else if (!gone) out[e.pos] = (out[e.pos] & 0xFFFFu) | ((uint32_t)off << 16);
    }
    extra.insert(extra.end(), bail_ops.begin(), bail_ops.end());
    std::sort(unsafe_bails.begin(), unsafe_bails.end());   // (log order = position order)
    for (size_t i = unsafe_bails.size(); i-- > 0;)   // (last first: earlier positions stay valid)
      out.erase(out.begin() + (long)unsafe_bails[i]->pos, out.begin() + (long)ends_at(*unsafe_bails[i]));
  }
  if (P) {
    // constant prefetch (gen_qsa.py NEXT_P): a constant handler whose predecessor is not itself
    // a prefetched one becomes its PF_ variant, and the predecessor's entry names its constant
    // (the dispatch of the predecessor loads it into CB); a PF_ handler whose successor is not
    // one re-loads its own constant (an in-flight load then writes CB's current contents)
    auto pf_kind = [](int kind) -> int {
      switch (kind) {
        case QK_PUSH_CONST: return QK_PF_PUSH_CONST;
        case QK_ADDC: return QK_PF_ADDC;
        case QK_SUBC: return QK_PF_SUBC;
        case QK_MULC: return QK_PF_MULC;
        case QK_BANDC: return QK_PF_BANDC;
        case QK_BORC: return QK_PF_BORC;
        case QK_BXORC: return QK_PF_BXORC;
        case QK_ADDCV: return QK_PF_ADDCV;
        case QK_SUBCV: return QK_PF_SUBCV;
        case QK_MULCV: return QK_PF_MULCV;
        case QK_BANDCV: return QK_PF_BANDCV;
        case QK_BORCV: return QK_PF_BORCV;
        case QK_BXORCV: return QK_PF_BXORCV;
        default: return -1;
      }
    };
    std::vector<char> pf(log.size(), 0);
    auto coff_bytes = [&](const Emit& e) -> uint32_t {
      const bool cv = e.kind == QK_ADDCV || e.kind == QK_SUBCV || e.kind == QK_MULCV || e.kind == QK_BANDCV ||
                      e.kind == QK_BORCV || e.kind == QK_BXORCV;
      return 4u * (cv ? (e.imm & 0xFFFFu) : e.imm);
    };
    for (size_t j = 1; j < log.size(); j++) {
      const Emit& e = log[j];
      const int fk = pf_kind(e.kind);
      if (fk < 0 || pf[j - 1] || qt.index[0][fk][e.d][e.v + 1] < 0) continue;
      pf[j] = 1;
      out[e.pos] = qt.hbase_lo[0] + qt.off[0][qt.index[0][fk][e.d][e.v + 1]];
      out[log[j - 1].pos + 2] = coff_bytes(e);
    }
    for (size_t j = 0; j < log.size(); j++)
      if (pf[j] && !(j + 1 < log.size() && pf[j + 1])) out[log[j].pos + 2] = coff_bytes(log[j]);
  }
  return x.consts.size() + extra.size() <= 0x10000u;
}

// A tape's low-limb prefilter program (CompiledTape::prog_pf) as P entries for frame mode 4:
// (handler address, the instruction's 32-bit immediate, 0).  PUSH_VAR and the bitwise ops are
// P's own handlers (on the narrow register map they act on eight blocks' low limbs).
// A PUSH_VAR read by the very next instruction is not an entry of its own: the reader's fused
// form takes the variable's registers in place (gen_qsa.py, the fused narrow handlers)
//   PUSH_VAR v1; PUSH_VAR v2; binop  ->  kind32VV / B*VV (x, v1), imm = 8 * v2
//   PUSH_VAR v; binop / EQ           ->  kind32V / B*V / EQ32V (d, v)
//   PUSH_VAR v; opK / EQK            ->  kindK32V (d, v), imm = k
// and a pattern whose handler the table lacks stays unfused.  MQ_PF_FUSE=0 (read per
// translation) turns the peephole off: one entry per instruction.
bool qsa_translate_pf(const QsaTable& qt, const CompiledTape& x, std::vector<uint32_t>& out) {
  out.clear();
  if (x.depth_pf > kQsaStackP) return false;
  const char* fe = std::getenv("MQ_PF_FUSE");
  const bool fuse = !(fe && fe[0] == '0' && fe[1] == 0);
  const size_t n = x.prog_pf.size() / 2;
  auto op_at = [&](size_t i) { return x.prog_pf[2 * i] & 0xFFu; };
  auto d_at = [&](size_t i) { return (int)((x.prog_pf[2 * i] >> 8) & 0xFu); };
  auto imm_at = [&](size_t i) { return x.prog_pf[2 * i + 1]; };
  auto emit = [&](int kind, int d, int v, uint32_t im) -> bool {
    if (d < 0 || d >= kQsaStackP || v < -1 || v >= kQsaVars) return false;
    const int h = qt.index[0][kind][d][v + 1];
    if (h < 0) return false;
    out.push_back(qt.hbase_lo[0] + qt.off[0][h]);
    out.push_back(im);
    out.push_back(0);
    return true;
  };
  // fused kinds of a reader whose right operand / both operands / only operand is a variable
  auto kind_v = [](uint32_t op) -> int {
    switch (op) {
      case PF_ADD: return QK_ADD32V;
      case PF_SUB: return QK_SUB32V;
      case PF_MUL: return QK_MUL32V;
      case PF_BAND: return QK_BANDV;
      case PF_BOR: return QK_BORV;
      case PF_BXOR: return QK_BXORV;
      case PF_EQ: return QK_EQ32V;
      default: return -1;
    }
  };
  auto kind_vv = [](uint32_t op) -> int {
    switch (op) {
      case PF_ADD: return QK_ADD32VV;
      case PF_SUB: return QK_SUB32VV;
      case PF_MUL: return QK_MUL32VV;
      case PF_BAND: return QK_BANDVV;
      case PF_BOR: return QK_BORVV;
      case PF_BXOR: return QK_BXORVV;
      default: return -1;
    }
  };
  auto kind_kv = [](uint32_t op) -> int {
    switch (op) {
      case PF_ADDK: return QK_ADDK32V;
      case PF_MULK: return QK_MULK32V;
      case PF_ANDK: return QK_ANDK32V;
      case PF_ORK: return QK_ORK32V;
      case PF_XORK: return QK_XORK32V;
      case PF_EQK: return QK_EQK32V;
      default: return -1;
    }
  };
  for (size_t i = 0; i < n; i++) {
    const uint32_t op = op_at(i), imm = imm_at(i);
    const int d = d_at(i);
    int kind = -1, v = -1;
    uint32_t im = imm;
    switch (op) {
      case PF_END: kind = QK_END; break;
      case PF_PUSH_VAR:
        if (imm >= (uint32_t)kQsaVars) return false;
        if (fuse && i + 2 < n && op_at(i + 1) == PF_PUSH_VAR && d_at(i + 1) == d + 1 && imm_at(i + 1) < (uint32_t)kQsaVars &&
            d_at(i + 2) == d + 1 && kind_vv(op_at(i + 2)) >= 0 && emit(kind_vv(op_at(i + 2)), d, (int)imm, 8u * imm_at(i + 1))) {
          i += 2;
          continue;
        }
        if (fuse && i + 1 < n && d_at(i + 1) == d) {
          const uint32_t nop = op_at(i + 1);
          if ((kind_v(nop) >= 0 && emit(kind_v(nop), d, (int)imm, 0)) ||
              (kind_kv(nop) >= 0 && emit(kind_kv(nop), d, (int)imm, imm_at(i + 1)))) {
            i += 1;
            continue;
          }
        }
        kind = QK_PUSH_VAR, v = (int)imm, im = 0;
        break;
      case PF_PUSH_K: kind = QK_PUSH_K32; break;
      case PF_ADD: kind = QK_ADD32; break;
      case PF_SUB: kind = QK_SUB32; break;
      case PF_MUL: kind = QK_MUL32; break;
      case PF_NEG: kind = QK_NEG32; break;
      case PF_BAND: kind = QK_BAND; break;
      case PF_BOR: kind = QK_BOR; break;
      case PF_BXOR: kind = QK_BXOR; break;
      case PF_BNOT: kind = QK_BNOT; break;
      case PF_ADDK: kind = QK_ADDK32; break;
      case PF_MULK: kind = QK_MULK32; break;
      case PF_ANDK: kind = QK_ANDK32; break;
      case PF_ORK: kind = QK_ORK32; break;
      case PF_XORK: kind = QK_XORK32; break;
      case PF_EQ: kind = QK_EQ32; break;
      case PF_EQK: kind = QK_EQK32; break;
      default: return false;
    }
    if (!emit(kind, kind == QK_END ? 0 : d, v, im)) return false;
  }
  return !out.empty();
}

// (P preloads variables 0-7 only: a program pushing any other variable is not tried on P)
bool p_candidate(const CompiledTape& x) {
  for (size_t pc = 0; pc < x.prog.size(); pc++) {
    const uint32_t op = x.prog[pc] & 0xFFu;
    if ((op == G_PUSH_VAR || op == G_PUSH_VAR_B) && (x.prog[pc] >> 12) >= (uint32_t)kQsaVars) return false;
    if (has_imm2(op)) pc++;
  }
  return true;
}

// Append a G program to `out`, whose next word is at position `pos` of its 64-word block: a
// handler group (word + inline data) that does not fit the rest of the block is preceded by
// REFILL and moves to the next block, the gap padded with END.
static void append_refilled(const QsaTable& qt, std::vector<uint32_t>& out, size_t& pos, const std::vector<uint32_t>& prog) {
  const std::vector<uint8_t>& data_words = qt.data_words;
  const uint32_t refill = hword(1, qt.off[1][qt.index[1][QK_REFILL][0][0]]);
  const uint32_t endw = hword(1, qt.off[1][qt.index[1][QK_END][0][0]]);
  for (size_t i = 0; i < prog.size();) {
    const size_t g = 1 + (size_t)data_words[prog[i] & 0xFFFFu];
    if (pos + g > 63) {
      out.push_back(refill);
      out.insert(out.end(), 63 - pos, endw);
      pos = 0;
    }
    for (size_t j = 0; j < g && i + j < prog.size(); j++) out.push_back(prog[i + j]);
    pos += g;
    i += g;
  }
}

// G programs stream through a 64-word VGPR window (gen_qsa.py NEXT_G): insert a REFILL word
// wherever the next handler word and its inline data would not fit in the current window (the
// refilled window starts right after the REFILL word).
void qsa_window_layout(const QsaTable& qt, std::vector<uint32_t>& prog) {
  // Windows are the program's aligned 64-word blocks: a handler group (word + inline data) that
  // does not fit the rest of a block is preceded by REFILL and moves to the next block (the gap
  // is padded with END), and the program is padded to a whole block.  So the window after the
  // current one is always 256 bytes further, which the kernel prefetches (gen_qsa.py NWIN), and
  // the programs of consecutive descriptors are contiguous blocks: the next tape's first window
  // is the prefetch of the current tape's last one.
  const uint32_t endw = hword(1, qt.off[1][qt.index[1][QK_END][0][0]]);
  std::vector<uint32_t> out;
  out.reserve(prog.size() + prog.size() / 32 + 64);
  size_t pos = 0;
  append_refilled(qt, out, pos, prog);
  if (pos) out.insert(out.end(), 64 - pos, endw);
  prog.swap(out);
}

// Column programs are short (C3: ~6 nodes): padding each to whole 64-word blocks made every column
// start with a window load, a memory round trip per column program (the G profile charged it to
// FRAME3: ~20 % of C3's cycles).  They are packed back to back instead: a program starts at the
// next word (or, when its first handler group would not fit the block, at the next block), the
// REFILL rule of qsa_window_layout applies inside it, and the kernel starts a program that lies in
// its current window without a load (gen_qsa.py load_window).  Returns the program's word offset;
// pos = the next word's position in its block.
uint32_t qsa_pack_program(const QsaTable& qt, std::vector<uint32_t>& out, size_t& pos, const std::vector<uint32_t>& prog) {
  const uint32_t endw = hword(1, qt.off[1][qt.index[1][QK_END][0][0]]);
  if (!prog.empty() && pos + 1 + (size_t)qt.data_words[prog[0] & 0xFFFFu] > 63) {
    out.insert(out.end(), 64 - pos, endw);
    pos = 0;
  }
  const uint32_t start = (uint32_t)out.size();
  append_refilled(qt, out, pos, prog);
  return start;
}

// Push counts of the variables (<= 256 bits) a set of compiled programs reads.
std::vector<int64_t> count_pushes(const ModelLayout& ml, const std::vector<CompiledTape>& cts,
                                  const std::vector<char>* skip) {
  std::vector<int64_t> pushes(ml.var_nl.size(), 0);
  for (size_t i = 0; i < cts.size(); i++) {
    if (skip && (*skip)[i]) continue;
    const auto& pr = cts[i].prog;
    for (size_t pc = 0; pc < pr.size(); pc++) {
      const uint32_t op = pr[pc] & 0xFFu, imm = pr[pc] >> 12;
      // (Bool variables with a lane mask are neither preloaded nor staged: PUSH_PKB)
      if ((op == G_PUSH_VAR || (op == G_PUSH_VAR_B && !(imm < ml.bmask_of_var.size() && ml.bmask_of_var[imm] >= 0))) &&
          imm < pushes.size() && ml.var_nl[imm] <= 8)
        pushes[imm]++;
      if (has_imm2(op)) pc++;
    }
  }
  return pushes;
}

// G kernel LDS staging plan: the most pushed variables (not preloaded) whose rows fit the
// workgroup's staging budget get consecutive LDS slots (gen_qsa.py stage_rows); their pushes
// become LDS reads.  Budget: MQ_G_STAGE_KB (default 26: the 80-VGPR G runs 6 waves per SIMD =
// 6 workgroups of 4 waves per CU, and 6 x 26 KB fit the CU's 160 KB; 40 KB, the budget of the
// 5-wave layout, capped C5 at 4 workgroups per CU: 70.5 vs 61.6 ms, profiles/r04c) KB per
// workgroup minus the temps of its 4 waves.  Every workgroup loads its rows
// once, so a variable is staged only when the workgroup's tapes (wg_share of the batch's
// programs) push it at least MQ_G_STAGE_MIN (default 1.5) times on average
// (profiles/r02t_*: 40 KB with no such floor sped C3 up and slowed C5, whose groups cover few
// tapes).  stage_rows is padded to a multiple of 8 with the zero row.
void plan_stage(const ModelLayout& ml, const std::vector<int64_t>& pushes, const std::vector<int>* gpre, int temps,
                double wg_share, std::vector<int>& gstage, std::vector<uint32_t>& rows) {
  int64_t kb = 26;
  if (const char* e = std::getenv("MQ_G_STAGE_KB")) kb = std::atol(e);
  double min_pushes = 1.5;
  if (const char* e = std::getenv("MQ_G_STAGE_MIN")) min_pushes = std::atof(e);
  const int64_t budget = (kb * 1024 - 4 * (int64_t)temps * 2048) / 256;
  gstage.assign(ml.var_nl.size(), -1);
  rows.clear();
  std::vector<int> order;
  for (size_t v = 0; v < pushes.size(); v++)
    if (pushes[v] > 0 && !(gpre && v < gpre->size() && (*gpre)[v] >= 0)) order.push_back((int)v);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pushes[a] > pushes[b]; });
  for (int v : order) {
    const int64_t nl = ml.var_nl[v];
    if ((double)pushes[v] * wg_share < min_pushes) break;   // (sorted by pushes)
    if ((int64_t)rows.size() + nl > budget) continue;
    gstage[v] = (int)rows.size();
    for (int64_t l = 0; l < nl; l++) rows.push_back(ml.var_off[v] + (uint32_t)l);
  }
  const uint32_t zero_row = ml.zero_row();
  while (rows.size() % 8) rows.push_back(zero_row);
}

}  // namespace mq
