// fc_plan.cpp — see fc_plan.h.  Host only: no HIP header, no context.
#include "fc_plan.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <set>

namespace mq {

// A program that is a flat conjunction of atoms (Bool variables, variable-constant compares),
// or the negation of one: ORs of atoms and of negated conjunctions are taken by De Morgan
// (OR(a, b) = NOT(AND(NOT a, NOT b))), the result negation returned in *neg.
// With `unary` (the two-phase kernel only) an atom may also compare a constant with a unary
// function of its variable: zero extension (free: values are canonical), sign extension, extract,
// shifts by constants, and division / remainder by small constants (FcXop, fc.hip fx_apply).
bool fc_match(const ModelLayout& ml, const CompiledTape& x, std::vector<uint32_t>& masks, std::vector<FcCmpH>& cmps,
              bool* neg, bool unary) {
  struct Item {
    int kind = 0;   // 0 model variable (BV, through xf), 1 constant, 2 conjunction (negated when neg)
    uint32_t v = 0;
    uint32_t w = 0;   // kind 0: the width of its current value
    bool neg = false;
    std::vector<uint32_t> m;
    std::vector<FcCmpH> q;
    std::vector<FcXop> xf;
  };
  // the 256-bit constant at word offset k of the tape's pool, limb by limb (8 limbs, zero padded)
  auto const_limbs = [&](uint32_t k, uint32_t out[8]) {
    for (int i = 0; i < 8; i++) out[i] = x.consts[k + i];
  };
  // value (< 2^32 or saturated) of a constant of width w: its limbs above 0 are zero?
  auto small_value = [&](const uint32_t l[8], uint64_t* v) {
    for (int i = 2; i < 8; i++)
      if (l[i]) return false;
    *v = (uint64_t)l[0] | ((uint64_t)l[1] << 32);
    return true;
  };
  // NOT of an item as a plain conjunction: a single atom negated, or a negated conjunction's body
  auto negate_to_conj = [](Item& a) -> bool {
    if (a.neg) {
      a.neg = false;
      return true;
    }
    if (a.m.size() + a.q.size() != 1) return false;
    if (!a.m.empty()) a.m[0] ^= 0x80000000u;
    else a.q[0].accept ^= 7u;
    return true;
  };
  std::vector<Item> st;
  const auto& pr = x.prog;
  auto bool_item = [&](uint32_t v, Item& it) {
    it.kind = 2;
    if (v < ml.bmask_of_var.size() && ml.bmask_of_var[v] >= 0) {
      it.m.push_back((uint32_t)ml.bmask_of_var[v]);
    } else {
      FcCmpH q{};
      q.row = ml.var_off[v];
      q.nl = 1;
      q.accept = kAccEq;
      q.c[0] = 1;
      it.q.push_back(q);
    }
  };
  for (size_t pc = 0; pc < pr.size(); pc++) {
    const uint32_t w = pr[pc], op = w & 0xFFu, imm = w >> 12;
    if (op == G_END) break;
    if (unary && op == G_CONCAT && pc + 1 < pr.size()) {
      // Concat(0, x): a zero extension (bitvec.py:16-22 pads a narrower operand so; EVM BYTE)
      const uint32_t w2 = pr[++pc];
      if (st.size() < 2 || st.back().kind != 0 || st[st.size() - 2].kind != 1 || st.back().w > imm || w2 > 256) return false;
      uint32_t hl[8];
      const_limbs(st[st.size() - 2].v, hl);
      for (int i = 0; i < 8; i++)
        if (hl[i]) return false;
      Item v = std::move(st.back());
      st.pop_back();
      st.back() = std::move(v);
      st.back().w = w2;
      continue;
    }
    if (unary && (op == G_EXTRACT || op == G_SEXT) && pc + 1 < pr.size()) {
      // (the two ops with a second word: the result width)
      const uint32_t w2 = pr[++pc];
      if (st.empty() || st.back().kind != 0 || st.back().xf.size() >= (size_t)kFcMaxXops) return false;
      Item& a = st.back();
      // (a value narrower than the op's operand was zero-extended: canonical values are, so the
      // op reads it at the wider width as is)
      if (op == G_EXTRACT) {
        if (imm + w2 > 256 || w2 == 0) return false;
        a.xf.push_back(FcXop{FX_EXTRACT | (std::max(a.w, imm + w2) << 8), imm, w2, 0});
      } else {
        if (imm < a.w || w2 <= imm || w2 > 256) return false;
        a.xf.push_back(FcXop{FX_SEXT | (imm << 8), w2, 0, 0});
      }
      a.w = w2;
      continue;
    }
    if (op == G_BAIL) {   // (a flat conjunction is too cheap to carry one; skipped all the same)
      pc++;
      continue;
    }
    if (has_imm2(op)) return false;
    Item it;
    switch (op) {
      case G_PUSH_VAR:
        if (imm >= ml.var_nl.size() || ml.var_width[imm] == 0 || ml.var_nl[imm] > 8) return false;
        it.kind = 0;
        it.v = imm;
        it.w = ml.var_width[imm];
        st.push_back(std::move(it));
        break;
      case G_LSHR: case G_SHL: case G_ASHR: case G_UREM: case G_UDIV: case G_SMOD: case G_SREM: case G_SDIV: {
        // a unary step: the variable (through its steps so far) OP a constant
        if (!unary || st.size() < 2 || st.back().kind != 1 || st[st.size() - 2].kind != 0) return false;
        const uint32_t kc = st.back().v;
        st.pop_back();
        Item& a = st.back();
        const uint32_t w = imm;   // (>= the value's width: a zero-extended value, read as is)
        if (imm < a.w || w == 0 || w > 256 || a.xf.size() >= (size_t)kFcMaxXops) return false;
        uint32_t l[8];
        const_limbs(kc, l);
        uint64_t k = 0;
        const bool small = small_value(l, &k);
        if (op == G_LSHR || op == G_SHL || op == G_ASHR) {
          const uint32_t sh = (!small || k >= w) ? w : (uint32_t)k;   // (>= w: the kernel's saturation)
          a.xf.push_back(FcXop{(op == G_LSHR ? FX_LSHR : op == G_SHL ? FX_SHL : FX_ASHR) | (w << 8), sh, 0, 0});
        } else if (op == G_UREM || op == G_UDIV) {
          if (!small || k == 0 || k >= (1u << 21)) return false;
          a.xf.push_back(FcXop{(op == G_UREM ? FX_UREM : FX_UDIV) | (w << 8), (uint32_t)k, 0, 0});
        } else {
          // signed divisor: |d| and its sign at width w (two's complement of the w-bit constant)
          bool dneg = ((l[(w - 1) / 32] >> ((w - 1) % 32)) & 1u) != 0;
          uint32_t m[8];
          for (int i = 0; i < 8; i++) m[i] = l[i];
          if (dneg) {   // |d| = -d mod 2^w
            uint64_t cy = 1;
            for (int i = 0; i < 8; i++) {
              const uint64_t t = (uint64_t)(~m[i]) + cy;
              m[i] = (uint32_t)t;
              cy = t >> 32;
            }
            for (int i = 0; i < 8; i++) {
              const uint32_t lo = 32u * i;
              if (w <= lo) m[i] = 0;
              else if (w < lo + 32) m[i] &= (1u << (w - lo)) - 1u;
            }
          }
          uint64_t ad = 0;
          if (!small_value(m, &ad) || ad == 0 || ad >= (1u << 21)) return false;
          const uint32_t code = op == G_SMOD ? FX_SMOD : op == G_SREM ? FX_SREM : FX_SDIV;
          a.xf.push_back(FcXop{code | (w << 8), (uint32_t)ad, dneg ? 1u : 0u, 0});
        }
        a.w = w;
        break;
      }
      case G_PUSH_VAR_B:
        if (imm >= ml.var_nl.size() || ml.var_width[imm] != 0) return false;
        bool_item(imm, it);
        st.push_back(std::move(it));
        break;
      case G_PUSH_CONST:
        if ((size_t)imm + 8 > x.consts.size()) return false;
        it.kind = 1;
        it.v = imm;
        st.push_back(std::move(it));
        break;
      case G_PUSH_BOOL:
        if (imm != 1) return false;
        it.kind = 2;   // TRUE: the empty conjunction
        st.push_back(std::move(it));
        break;
      case G_NOT: {
        if (st.empty() || st.back().kind != 2) return false;
        Item& a = st.back();
        if (!negate_to_conj(a)) a.neg = true;   // NOT of a conjunction of several atoms
        break;
      }
      case G_AND: case G_OR: {
        if (st.size() < 2 || st.back().kind != 2 || st[st.size() - 2].kind != 2) return false;
        Item b = std::move(st.back());
        st.pop_back();
        Item& a = st.back();
        if (op == G_OR) {   // NOT(AND(NOT a, NOT b))
          if (!negate_to_conj(a) || !negate_to_conj(b)) return false;
          a.neg = true;
        } else if (a.neg || b.neg) {
          return false;
        }
        a.m.insert(a.m.end(), b.m.begin(), b.m.end());
        a.q.insert(a.q.end(), b.q.begin(), b.q.end());
        break;
      }
      case G_EQ: case G_ULT: case G_ULE: case G_UGT: case G_UGE:
      case G_SLT: case G_SLE: case G_SGT: case G_SGE: {
        if (st.size() < 2) return false;
        Item r = std::move(st.back());
        st.pop_back();
        Item l = std::move(st.back());
        st.pop_back();
        bool swap;
        if (l.kind == 0 && r.kind == 1) swap = false;
        else if (l.kind == 1 && r.kind == 0) swap = true;
        else if (unary && l.kind == 1 && r.kind == 1 && imm > 0 && imm <= 256 && !ml.var_off.empty()) {
          // two constants (an unfolded compare): its truth value — TRUE is the empty
          // conjunction, FALSE an atom that accepts nothing
          uint32_t a[8], b[8];
          const_limbs(l.v, a);
          const_limbs(r.v, b);
          if (op >= G_SLT) {
            a[(imm - 1) / 32] ^= 1u << ((imm - 1) % 32);
            b[(imm - 1) / 32] ^= 1u << ((imm - 1) % 32);
          }
          int cmp = 0;
          for (int i = 7; i >= 0 && !cmp; i--) cmp = a[i] < b[i] ? -1 : (a[i] > b[i] ? 1 : 0);
          bool t;
          switch (op) {
            case G_EQ: t = cmp == 0; break;
            case G_ULT: case G_SLT: t = cmp < 0; break;
            case G_ULE: case G_SLE: t = cmp <= 0; break;
            case G_UGT: case G_SGT: t = cmp > 0; break;
            default: t = cmp >= 0; break;
          }
          it.kind = 2;
          if (!t) {
            FcCmpH q{};
            q.row = ml.var_off[0];
            q.nl = 1;
            q.accept = 0;
            it.q.push_back(q);
          }
          st.push_back(std::move(it));
          break;
        } else {
          return false;
        }
        const Item& var = swap ? r : l;
        const Item& cst = swap ? l : r;
        const uint32_t wdt = imm;
        // (a narrower value compared at a wider width: a zero-extended column read, free)
        if (wdt == 0 || wdt > 256 || var.w > wdt || (!unary && (var.w != wdt || !var.xf.empty()))) return false;
        FcCmpH q{};
        q.row = ml.var_off[var.v];
        q.nl = (wdt + 31) / 32;
        q.src_nl = ml.var_nl[var.v];
        q.nx = (uint32_t)var.xf.size();
        for (size_t k = 0; k < var.xf.size(); k++) q.xf[k] = var.xf[k];
        for (uint32_t i = 0; i < q.nl; i++) q.c[i] = x.consts[cst.v + i];
        // x OP c with the variable on the left; a constant on the left mirrors the order
        switch (op) {
          case G_EQ: q.accept = kAccEq; break;
          case G_ULT: case G_SLT: q.accept = swap ? kAccGt : kAccLt; break;
          case G_ULE: case G_SLE: q.accept = swap ? kAccGe : kAccLe; break;
          case G_UGT: case G_SGT: q.accept = swap ? kAccLt : kAccGt; break;
          default: q.accept = swap ? kAccLe : kAccGe; break;
        }
        if (op >= G_SLT) {   // signed: flip the sign bit of both sides, then compare unsigned
          q.f[q.nl - 1] = 1u << ((wdt - 1) % 32);
          q.c[q.nl - 1] ^= q.f[q.nl - 1];
        }
        it.kind = 2;
        it.q.push_back(q);
        st.push_back(std::move(it));
        break;
      }
      default:
        return false;
    }
  }
  if (st.size() != 1 || st[0].kind != 2) return false;
  if (st[0].neg && !neg) return false;
  if (neg) *neg = st[0].neg;
  masks.insert(masks.end(), st[0].m.begin(), st[0].m.end());
  cmps.insert(cmps.end(), st[0].q.begin(), st[0].q.end());
  return true;
}

void fc_plan(const ModelLayout& ml, const std::vector<std::vector<uint32_t>>& fm, const std::vector<std::vector<FcCmpH>>& fq,
             const std::vector<char>& negated, std::vector<char>& keep, const std::function<uint32_t(size_t)>& out_of,
             const std::function<int32_t(size_t)>& mask_out,
             const std::function<std::pair<uint32_t, uint32_t>(size_t)>& nodes_ops, FcPlan& P) {
  const uint32_t zero_row = ml.zero_row();
  std::map<uint32_t, int64_t> row_use, mask_use;
  std::map<uint32_t, uint32_t> row_nl;
  for (size_t i = 0; i < keep.size(); i++) {
    if (!keep[i]) continue;
    for (const auto& q : fq[i]) {
      row_use[q.row]++;
      row_nl[q.row] = q.nl;
    }
    for (uint32_t e : fm[i]) mask_use[e & 0x7FFFFFFFu]++;
  }
  auto by_use = [](const std::map<uint32_t, int64_t>& u) {
    std::vector<std::pair<int64_t, uint32_t>> o;
    for (const auto& kv : u) o.push_back({kv.second, kv.first});
    std::stable_sort(o.begin(), o.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    return o;
  };
  std::map<uint32_t, uint32_t> slot_of, mslot_of;
  for (const auto& o : by_use(row_use)) {
    const uint32_t nl = row_nl[o.second], width = nl <= 2 ? 2 : 8;   // (padded with the zero row)
    if (P.stage_rows.size() + width > (size_t)kFcStageRows) continue;
    slot_of[o.second] = (uint32_t)P.stage_rows.size();
    for (uint32_t l = 0; l < width; l++) P.stage_rows.push_back(l < nl ? o.second + l : zero_row);
  }
  for (const auto& o : by_use(mask_use)) {
    if (P.stage_masks.size() >= (size_t)kFcStageMasks) break;
    mslot_of[o.second] = (uint32_t)P.stage_masks.size();
    P.stage_masks.push_back(o.second);
  }
  P.prefix.assign(2, 0);
  for (size_t i = 0; i < keep.size(); i++) {
    if (!keep[i]) continue;
    bool ok = true;
    for (const auto& q : fq[i]) ok = ok && slot_of.count(q.row);
    for (uint32_t e : fm[i]) ok = ok && mslot_of.count(e & 0x7FFFFFFFu);
    if (!ok) {
      keep[i] = 0;
      continue;
    }
    FcTape f{};
    f.out = out_of(i);
    f.mask_out = mask_out(i);
    f.mask_off = (uint32_t)P.mask_lds.size();
    f.n_mask = (uint32_t)fm[i].size() | (negated[i] ? 0x80000000u : 0u);
    for (uint32_t e : fm[i]) P.mask_lds.push_back(8u * mslot_of[e & 0x7FFFFFFFu] | (e >> 31));
    if (!fm[i].empty())
      while (P.mask_lds.size() % 16) P.mask_lds.push_back(P.mask_lds.back());   // (the same AND again)
    f.cmp_off = (uint32_t)P.cmps.size();
    f.n_cmp = (uint32_t)fq[i].size();
    for (const auto& h : fq[i]) {
      FcCmp q{};
      q.h.slot = slot_of[h.row];
      q.h.nl = h.nl;
      q.h.accept = h.accept;
      q.h.c01 = (uint64_t)h.c[0] | ((uint64_t)h.c[1] << 32);
      q.h.f01 = (uint64_t)h.f[0] | ((uint64_t)h.f[1] << 32);
      for (int l = 0; l < 6; l++) {
        q.t.c[l] = h.c[2 + l];
        q.t.f[l] = h.f[2 + l];
      }
      P.cmps.push_back(q);
    }
    const auto no = nodes_ops(i);
    f.n_nodes = no.first;
    f.alg_ops = no.second;
    P.tapes.push_back(f);
    P.prefix.push_back(P.prefix[P.prefix.size() - 2] + f.n_nodes);
    P.prefix.push_back(P.prefix[P.prefix.size() - 2] + f.alg_ops);
  }
}

void fca_plan(const ModelLayout& ml, const std::vector<std::vector<uint32_t>>& fm, const std::vector<std::vector<FcCmpH>>& fq,
              const std::vector<char>& negated, std::vector<char>& keep, const std::function<uint32_t(size_t)>& out_of,
              const std::function<std::pair<uint32_t, uint32_t>(size_t)>& nodes_ops, FcaPlan& P,
              const std::function<int32_t(size_t)>& mask_out) {
  const uint32_t zero_row = ml.zero_row();
  // key: row, source limbs, path (1: the 8-limb path — wide compares, zero-extended reads wider
  // than 64 bits, unary atoms), accept, compare limbs, then the constant / flip limbs and the
  // transform steps (atoms of one (row, source limbs, path) form groups)
  auto atom_key = [](const FcCmpH& h, bool* ng) {
    *ng = h.accept >= 4;
    const uint32_t src = h.src_nl ? h.src_nl : h.nl;
    const uint32_t general = (h.nx > 0 || h.nl > 2 || src > 2) ? 1u : 0u;
    std::vector<uint32_t> key{h.row, src, general, *ng ? (h.accept ^ 7u) : h.accept, h.nl, h.nx};
    for (uint32_t l = 0; l < h.nl; l++) {
      key.push_back(h.c[l]);
      key.push_back(h.f[l]);
    }
    for (uint32_t k = 0; k < h.nx; k++) {
      key.push_back(h.xf[k].code);
      key.push_back(h.xf[k].p0);
      key.push_back(h.xf[k].p1);
      key.push_back(h.xf[k].p2);
    }
    return key;
  };
  // the segment being built: its atoms / masks in arrival order, and its tapes' symbolic entries
  // (kind 0 mask slot, 1 atom; local id; negated)
  struct Ent {
    uint32_t kind, id, neg;
  };
  std::map<std::vector<uint32_t>, uint32_t> atom_of;
  std::vector<std::vector<uint32_t>> akeys;
  std::map<uint32_t, uint32_t> mask_of;
  std::vector<uint32_t> masks;
  std::vector<std::vector<Ent>> tl;
  std::vector<size_t> tsrc;
  P.chunk_off.assign(1, 0);
  auto close = [&]() {
    if (tl.empty()) return;
    FcaPlanSeg sg{};
    sg.atom_off = (int)P.atoms.size();
    sg.n_atoms = (int)akeys.size();
    sg.group_off = (int)P.groups.size();
    sg.tape_first = (int)P.tape_out.size();
    sg.n_tapes = (int)tl.size();
    sg.chunk_first = (int)P.chunk_off.size() - 1;
    sg.smask_off = (int)P.stage_masks.size();
    sg.n_smask = (int)masks.size();

    // atoms ordered by (variable row, limbs): groups
    std::vector<uint32_t> ord(akeys.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = (uint32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
      for (int f = 0; f < 3; f++)
        if (akeys[x][f] != akeys[y][f]) return akeys[x][f] < akeys[y][f];
      return false;
    });
    static const uint32_t group_atoms = [] {
      const char* e = std::getenv("MQ_FCA_GROUP_ATOMS");
      return e ? (uint32_t)std::max(1, std::atoi(e)) : (uint32_t)kFcaGroupAtoms;
    }();
    std::vector<uint32_t> pos(akeys.size());
    for (size_t r = 0; r < ord.size(); r++) {
      const std::vector<uint32_t>& key = akeys[ord[r]];
      pos[ord[r]] = (uint32_t)r;
      // (a group holds at most kFcaGroupAtoms atoms: the 4 waves take every fourth group, so one
      // variable's many compares must not land on one wave)
      if (r == 0 || akeys[ord[r - 1]][0] != key[0] || akeys[ord[r - 1]][1] != key[1] ||
          akeys[ord[r - 1]][2] != key[2] || P.groups.back().count >= group_atoms) {
        FcaGroup g{};
        const uint32_t nl = key[1];
        for (uint32_t l = 0; l < 8; l++) g.rows[l] = l < nl ? key[0] + l : zero_row;
        g.first = (uint32_t)r;
        g.nl = key[2] ? 8u : nl;   // (the kernel's 8-limb path for nl > 2)
        P.groups.push_back(g);
      }
      P.groups.back().count++;
      FcCmp q{};
      q.h.slot = 0;
      const uint32_t cnl = key[4], nx = key[5];
      q.h.nl = cnl;
      q.h.accept = key[3];
      uint32_t cc[8] = {0}, ff[8] = {0};
      for (uint32_t l = 0; l < cnl; l++) {
        cc[l] = key[6 + 2 * l];
        ff[l] = key[7 + 2 * l];
      }
      FcXf xf{};
      xf.n = nx;
      for (uint32_t k = 0; k < nx; k++) {
        const size_t o = 6 + 2 * cnl + 4 * k;
        xf.op[k] = FcXop{key[o], key[o + 1], key[o + 2], key[o + 3]};
      }
      P.xfs.push_back(xf);
      P.any_xf |= nx > 0;
      q.h.c01 = (uint64_t)cc[0] | ((uint64_t)cc[1] << 32);
      q.h.f01 = (uint64_t)ff[0] | ((uint64_t)ff[1] << 32);
      for (int l = 0; l < 6; l++) {
        q.t.c[l] = cc[2 + l];
        q.t.f[l] = ff[2 + l];
      }
      P.atoms.push_back(q);
    }
    sg.n_groups = (int)P.groups.size() - sg.group_off;
    P.stage_masks.insert(P.stage_masks.end(), masks.begin(), masks.end());
    const uint32_t abase = 1u + (uint32_t)masks.size();
    // chunks of 64 tapes, entries k-major; short lists padded with entry 0 (all ones)
    for (size_t c0 = 0; c0 < tl.size(); c0 += 64) {
      size_t kmax = 0;
      for (size_t t = c0; t < std::min(tl.size(), c0 + 64); t++) kmax = std::max(kmax, tl[t].size());
      for (size_t k = 0; k < kmax; k++)
        for (size_t l = 0; l < 64; l++) {
          const size_t t = c0 + l;
          uint32_t e = 0;
          if (t < tl.size() && k < tl[t].size()) {
            const Ent& x = tl[t][k];
            e = (x.kind == 0 ? 1u + x.id : abase + pos[x.id]) | (x.neg ? 0x80000000u : 0u);
          }
          P.lists.push_back(e);
        }
      P.chunk_off.push_back((uint32_t)P.lists.size());
    }
    for (size_t t = 0; t < tl.size(); t++) {
      P.tape_out.push_back(out_of(tsrc[t]) | (negated[tsrc[t]] ? 0x80000000u : 0u));
      const auto no = nodes_ops(tsrc[t]);
      P.metric.push_back(no.first);
      P.metric.push_back(no.second);
      if (mask_out) P.col_mask.push_back(mask_out(tsrc[t]));
    }
    P.segs.push_back(sg);
    atom_of.clear();
    akeys.clear();
    mask_of.clear();
    masks.clear();
    tl.clear();
    tsrc.clear();
  };
  for (size_t i = 0; i < keep.size(); i++) {
    if (!keep[i]) continue;
    if (fq[i].size() > (size_t)kFcaMaxAtoms || fm[i].size() > (size_t)kFcStageMasks) {
      keep[i] = 0;
      continue;
    }
    // this tape's new atoms / masks; a new segment when they do not fit
    size_t new_a = 0, new_m = 0;
    {
      std::set<std::vector<uint32_t>> fa;
      std::set<uint32_t> fmk;
      for (const auto& h : fq[i]) {
        bool ng;
        auto key = atom_key(h, &ng);
        if (!atom_of.count(key)) fa.insert(key);
      }
      for (uint32_t e : fm[i])
        if (!mask_of.count(e & 0x7FFFFFFFu)) fmk.insert(e & 0x7FFFFFFFu);
      new_a = fa.size();
      new_m = fmk.size();
    }
    if (akeys.size() + new_a > (size_t)kFcaMaxAtoms || masks.size() + new_m > (size_t)kFcStageMasks) close();
    std::vector<Ent> ent;
    for (uint32_t e : fm[i]) {
      const uint32_t v = e & 0x7FFFFFFFu;
      auto it = mask_of.find(v);
      uint32_t id;
      if (it == mask_of.end()) {
        id = (uint32_t)masks.size();
        mask_of[v] = id;
        masks.push_back(v);
      } else {
        id = it->second;
      }
      ent.push_back(Ent{0, id, e >> 31});
    }
    for (const auto& h : fq[i]) {
      bool ng;
      auto key = atom_key(h, &ng);
      auto it = atom_of.find(key);
      uint32_t id;
      if (it == atom_of.end()) {
        id = (uint32_t)akeys.size();
        atom_of[key] = id;
        akeys.push_back(key);
      } else {
        id = it->second;
      }
      ent.push_back(Ent{1, id, ng ? 1u : 0u});
    }
    tl.push_back(std::move(ent));
    tsrc.push_back(i);
  }
  close();
}

// Latency weight of a G program on one tile: its ops, plus the round trips of its variable
// pushes and table lookups (a store chain's select ends in a lookup; these dominate a column level)
double g_cost(const CompiledTape& x) {
  double w = 0;
  for (size_t pc = 0; pc < x.prog.size(); pc++) {
    const uint32_t op = x.prog[pc] & 0xFFu;
    w += 1;
    if (op == G_PUSH_VAR || op == G_PUSH_VAR_B) w += 4;
    if (op == G_UF1 || op == G_UF2 || op == G_UFK0 || op == G_UFK || op == G_UFKV) w += 24;
    if (has_imm2(op)) pc++;
  }
  return w;
}

// Split a column level's G programs into groups (a group = one wave of G on one tile; group g
// = descriptors [tab[g], tab[g+1]), the table gen_qsa.py's mode-3 prologue reads) so the
// heaviest group is as light as it can be: longest processing time first over
// min(n, ceil(n / tpg) rounded up to the workgroup's 4 waves) groups, of any sizes.  A workgroup
// holds its LDS until its slowest wave ends, so a level's time follows its heaviest group (C4
// level 2, five store chains: three in one wave of three 0.69 ms; 2-2-1 0.50 ms).  Reorders idx
// group by group; tab gets groups rounded up to 4, + 1 entries (empty groups past the last).
void balance_groups(const std::vector<CompiledTape>& ct, std::vector<int>& idx, int tpg,
                    std::vector<uint32_t>& tab) {
  const int n = (int)idx.size();
  const int groups = std::max(1, std::min(n, ((n + tpg - 1) / tpg + 3) / 4 * 4));
  std::vector<std::pair<double, int>> w;
  for (int i : idx) w.push_back({g_cost(ct[i]), i});
  std::stable_sort(w.begin(), w.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
  std::vector<double> load(groups, 0);
  std::vector<std::vector<int>> members(groups);
  for (const auto& x : w) {
    int best = 0;
    for (int g = 1; g < groups; g++)
      if (load[g] < load[best]) best = g;
    members[best].push_back(x.second);
    load[best] += x.first;
  }
  idx.clear();
  tab.assign(1, 0);
  for (const auto& m : members) {
    idx.insert(idx.end(), m.begin(), m.end());
    tab.push_back((uint32_t)idx.size());
  }
  while ((tab.size() - 1) % 4) tab.push_back((uint32_t)n);
}

}  // namespace mq
