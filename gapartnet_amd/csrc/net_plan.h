// net_plan.h — what a pass of the layer-program executor (net.hip, which alone includes this file) decides before its first
// launch: who reads which slot, which BatchNorms ride in which conv launches, where everything lives in the workspace, and
// whether the tables are fit to run at all.  Host code only: nothing here launches or touches the device.
#pragma once
#include <algorithm>
#include <vector>

#include "gpn_common.h"
#include "net_wgrad.h"  // kWgradBatchBytes

namespace {
// One or two networks per pass.  Two ("paired" passes, include/gpn.h): structurally identical programs over the SAME rulebooks
// whose layers are launched TOGETHER: every conv / BatchNorm-apply / concat launch computes layer i of both networks (blockIdx.y
// picks the network's pointer set: gpn::ConvTwin, gpn::BnFwdPtrs).  The arithmetic of each network is that of its own single pass.
struct NetSet {
  gpn_net_slot_t* slots;
  const gpn_net_conv_t* convs;
  const gpn_net_bn_t* bns;
};
// the tables of a pass, as the entry points receive them (shapes are read from the first network's tables)
struct Program {
  const char* who;
  const gpn_net_op_t* ops;
  int n_ops;
  const NetSet* nets;
  int n_nets, n_slots;
  const gpn_net_rulebook_t* rbs;
  int n_rbs, n_convs, n_bns;
};
inline size_t slot_bytes(const gpn_net_slot_t& s) { return (size_t)s.rows * s.channels * sizeof(float); }
inline gpn::DevRows dev_rows(const gpn_net_slot_t& s) { return gpn::DevRows{s.rows_dev, s.rows_plan}; }
inline int64_t plan_of(const gpn_net_slot_t& s) { return gpn::plan_rows(s.rows, dev_rows(s)); }
constexpr size_t kNoBuffer = ~(size_t)0;  // "none" among byte offsets

// ---- program analysis: who reads and writes which slot --------------------------------------------------------------------
struct Analysis {
  std::vector<int> readers;       // by slot: ops that read it
  std::vector<int> first_reader;  // by slot: the first op (program order) that reads it, or -1
  std::vector<int> producer;      // by slot: the first op that writes it, or -1
};
Analysis analyse(const gpn_net_op_t* ops, int n_ops, int n_slots) {  // (slot indices are in range: check_program / plan_bf16)
  Analysis a{std::vector<int>(n_slots, 0), std::vector<int>(n_slots, -1), std::vector<int>(n_slots, -1)};
  for (int i = n_ops - 1; i >= 0; --i) {
    a.readers[ops[i].src0]++, a.first_reader[ops[i].src0] = i;
    if (ops[i].src1 >= 0) a.readers[ops[i].src1]++, a.first_reader[ops[i].src1] = i;
    a.producer[ops[i].dst] = i;
  }
  return a;
}
// BN op i + 1 directly follows CONV op i and is the sole reader of its output: the conv launch can do work for that BatchNorm
inline bool bn_follows_conv(const gpn_net_op_t* ops, int n_ops, int i, const Analysis& a) {
  return i + 1 < n_ops && ops[i].kind == GPN_NET_CONV && ops[i + 1].kind == GPN_NET_BN && ops[i + 1].src0 == ops[i].dst &&
         a.readers[ops[i].dst] == 1;
}
// a FOLD (the conv launch writes the BatchNorm's output slot instead of its own) must not write what it reads, nor take the
// unwritten conv output as the residual
inline bool fold_aliases(const gpn_net_op_t& conv, const gpn_net_op_t& bn) { return bn.src1 == conv.dst || bn.dst == conv.src0; }

// ---- forward and backward plans ---------------------------------------------------------------------------------------------
struct FwdPlan {
  // training: a BatchNorm that directly follows a conv whose kernel has the sum epilogue gets its statistics from that launch
  // (bn_stats.h) and keeps only its apply pass.  By CONV op and by the BN op behind it: byte offset of the slab the sums are
  // accumulated in, within a network's stat slabs (kNoBuffer = none); slab_bytes of them are zeroed at the start of the pass
  std::vector<size_t> slab;
  size_t slab_bytes = 0;
  // inference: a BatchNorm that directly follows a conv on a kernel with the affine epilogue is applied by that conv's launch
  // (gpn::ConvAffine: the same bits) and has no launch of its own; the conv's own output slot stays unwritten.
  std::vector<char> folded;  // folded[i] != 0: BN op i is applied by CONV op i - 1
};
// mode: 0 = eval (running statistics), 1 = training (batch statistics), GPN_NET_INFERENCE = eval and no backward pass follows
FwdPlan plan_forward(const Program& p, int mode, bool fusion) {
  FwdPlan f;
  f.slab.assign(p.n_ops, kNoBuffer);
  f.folded.assign(p.n_ops, 0);
  if (!fusion || mode == 0) return f;
  const Analysis a = analyse(p.ops, p.n_ops, p.n_slots);
  for (int i = 0; i < p.n_ops; ++i) {
    if (!bn_follows_conv(p.ops, p.n_ops, i, a)) continue;
    const gpn_net_op_t &cv_op = p.ops[i], &bn_op = p.ops[i + 1];
    const gpn_net_rulebook_t& rb = p.rbs[cv_op.rulebook];
    const gpn_net_conv_t& cv = p.nets[0].convs[cv_op.param];
    const gpn_net_slot_t& out_slot = p.nets[0].slots[cv_op.dst];
    const gpn::ConvRoute route = gpn::spconv_fwd_route(rb.K, rb.n_dst, cv.cin, cv.cout, dev_rows(out_slot));
    if (mode == 1) {
      if (!gpn::bn_two_pass(plan_of(out_slot), cv.cout) || !route.sums) continue;
      f.slab[i] = f.slab[i + 1] = f.slab_bytes;
      f.slab_bytes += gpn::stat_slab_bytes(cv.cout);
    } else {
      bool ok = route.affine && !fold_aliases(cv_op, bn_op);  // (one launch has one eps: the two networks' must agree)
      for (int t = 1; t < p.n_nets; ++t) ok = ok && p.nets[t].bns[bn_op.param].eps == p.nets[0].bns[bn_op.param].eps;
      f.folded[i + 1] = ok;
    }
  }
  return f;
}

struct BwdPlan {
  // A dgrad conv that writes the FINAL gradient of a BatchNorm's output (it is the slot's first reader in program order, so
  // the last one of the reverse walk) adds that BatchNorm's backward sums in its epilogue (bn_stats.h); the BatchNorm then
  // runs only its apply pass.  fused_by[i]: the BN op CONV op i accumulates for, or -1
  std::vector<int> fused_by;
  std::vector<size_t> slab;  // by BN op: byte offset of its slab within a network's stat slabs (kNoBuffer = none)
  size_t slab_bytes = 0;
};
BwdPlan plan_backward(const Program& p, int need_input_grad, bool fusion) {
  BwdPlan b;
  b.fused_by.assign(p.n_ops, -1);
  b.slab.assign(p.n_ops, kNoBuffer);
  if (!fusion) return b;
  const Analysis a = analyse(p.ops, p.n_ops, p.n_slots);
  for (int i = 0; i < p.n_ops; ++i) {
    const gpn_net_op_t& op = p.ops[i];
    if (op.kind != GPN_NET_CONV) continue;
    const int j = a.producer[op.src0];
    if (j < 0 || p.ops[j].kind != GPN_NET_BN || a.first_reader[op.src0] != i) continue;
    if (op.src0 == 0 && !need_input_grad) continue;  // (no dgrad launch)
    const gpn_net_rulebook_t& rb = p.rbs[op.rulebook];
    const gpn_net_conv_t& cv = p.nets[0].convs[op.param];
    const gpn_net_slot_t& in_slot = p.nets[0].slots[op.src0];
    if (!gpn::bn_two_pass(plan_of(in_slot), cv.cin) || !gpn::spconv_fwd_route(rb.K, rb.n_src, cv.cout, cv.cin, dev_rows(in_slot)).sums)
      continue;
    b.slab[j] = b.slab_bytes;
    b.slab_bytes += gpn::stat_slab_bytes(cv.cin);
    b.fused_by[i] = j;
  }
  return b;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
struct Need {
  size_t tmp = 0;     // gradient staging buffer (largest slot that can receive a second gradient)
  size_t op = 0;      // largest per-op workspace of the main chain (conv tap-split partials, BN partials)
  size_t wgrad = 0;   // weight-gradient partials (side stream): room for a batch of layers whose slice sums run in one launch
  size_t packed = 0;  // all packed weights of the program
  size_t stats = 0;   // BatchNorm sum slabs the conv epilogues add to (bn_stats.h), one per BN op
};
Need workspace_need(const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, const gpn_net_rulebook_t* rbs,
                    const gpn_net_conv_t* convs) {
  Need n;
  size_t wgrad_sum = 0;
  for (int i = 0; i < n_ops; ++i) {
    const gpn_net_op_t& op = ops[i];
    const gpn_net_slot_t& s0 = slots[op.src0];
    if (op.kind == GPN_NET_CONV) {
      const gpn_net_rulebook_t& rb = rbs[op.rulebook];
      const gpn_net_conv_t& cv = convs[op.param];
      size_t w = gpn_spconv_fwd_ws_bytes(rb.K, rb.n_dst, cv.cin, cv.cout);
      size_t wt = gpn_spconv_fwd_ws_bytes(rb.K, rb.n_src, cv.cout, cv.cin);
      n.op = std::max(n.op, std::max(w, wt));
      const size_t wg = gpn_spconv_wgrad_ws_bytes(rb.K, cv.cin, cv.cout, rb.n_dst);
      n.wgrad = std::max(n.wgrad, wg);
      wgrad_sum += wg;
      n.packed += gpn::align_up((size_t)rb.K * cv.cin * cv.cout * sizeof(float));
      n.tmp = std::max(n.tmp, slot_bytes(s0));
    } else if (op.kind == GPN_NET_BN) {
      n.op = std::max(n.op, gpn_bn_ws_bytes(s0.rows, s0.channels));
      n.stats += gpn::stat_slab_bytes(s0.channels);
      if (op.src1 >= 0) n.tmp = std::max(n.tmp, slot_bytes(slots[op.src1]));
    }
  }
  n.tmp = gpn::align_up(n.tmp);
  n.op = gpn::align_up(n.op);
  n.wgrad = gpn::align_up(std::max(n.wgrad, std::min(wgrad_sum, kWgradBatchBytes)));
  return n;
}

// Where a pass keeps what in the caller's workspace:
//   forward:   per network [packed weights | stat slabs], then the per-op workspace (which takes the rest)
//   backward:  per network [staging | packed weights | stat slabs], then need.op of per-op workspace, then the weight-gradient
//              workspace (n_nets x need.wgrad; it takes the rest).  gpn_net_ws_bytes is the backward total of ONE network.
struct Layout {
  Need need;
  int n_nets;
  bool backward;
  char* base;  // the caller's workspace (nullptr: only total() is asked for)
  size_t ws_bytes;
  size_t per_net() const { return (backward ? need.tmp : 0) + need.packed + need.stats; }
  float* staging(int t) const { return reinterpret_cast<float*>(base + t * per_net()); }  // (backward only)
  char* packed(int t) const { return base + t * per_net() + (backward ? need.tmp : 0); }
  char* stats(int t) const { return packed(t) + need.packed; }
  unsigned long long* slab(int t, size_t off) const {  // a plan's slab offset -> the slab of network t
    return off == kNoBuffer ? nullptr : reinterpret_cast<unsigned long long*>(stats(t) + off);
  }
  char* op_ws() const { return base + n_nets * per_net(); }
  size_t op_ws_bytes() const { return backward ? need.op : ws_bytes - n_nets * per_net(); }
  char* wgrad_ws() const { return op_ws() + need.op; }  // (backward only)
  size_t wgrad_ws_bytes() const { return ws_bytes - (n_nets * per_net() + need.op); }
  size_t total() const { return n_nets * per_net() + need.op + (backward ? n_nets * need.wgrad : 0); }
};
// the layout of a pass, or GPN_ERR_WS: the last check before the first launch
int layout_of(const Program& p, bool backward, void* ws, size_t ws_bytes, Layout& lay) {
  lay = Layout{workspace_need(p.ops, p.n_ops, p.nets[0].slots, p.rbs, p.nets[0].convs), p.n_nets, backward, static_cast<char*>(ws), ws_bytes};
  if (ws && ws_bytes >= lay.total()) return GPN_OK;
  gpn::set_error("%s: workspace too small (%zu needed, %zu given)", p.who, lay.total(), ws_bytes);
  return GPN_ERR_WS;
}

// ---- validation, all of it before the first launch of a pass.  check_program: indices, shapes, rulebook / weight pointers ----
int bad_op(const Program& p, int i, const char* what) {
  gpn::set_error("%s: op %d (kind %d): %s", p.who, i, p.ops[i].kind, what);
  return GPN_ERR_ARG;
}
int check_program(const Program& p) {
  for (int t = 0; t < p.n_nets; ++t) {
    const auto [slots, convs, bns] = p.nets[t];
    if (!p.ops || !slots || p.n_ops < 0 || p.n_slots < 1 || (p.n_rbs && !p.rbs) || (p.n_convs && !convs) || (p.n_bns && !bns)) {
      gpn::set_error("%s: null table", p.who);
      return GPN_ERR_ARG;
    }
    for (int i = 0; i < p.n_ops; ++i) {
      const gpn_net_op_t& op = p.ops[i];
      if (op.src0 < 0 || op.src0 >= p.n_slots || op.dst < 0 || op.dst >= p.n_slots || op.src1 >= p.n_slots) return bad_op(p, i, "slot index out of range");
      const gpn_net_slot_t &s0 = slots[op.src0], &d = slots[op.dst];
      if (s0.rows < 1 || d.rows < 1) return bad_op(p, i, "empty slot");
      if (op.kind == GPN_NET_CONV) {
        if (op.rulebook < 0 || op.rulebook >= p.n_rbs || op.param < 0 || op.param >= p.n_convs) return bad_op(p, i, "table index out of range");
        const gpn_net_rulebook_t& rb = p.rbs[op.rulebook];
        const gpn_net_conv_t& cv = convs[op.param];
        if (rb.n_src != s0.rows || rb.n_dst != d.rows || cv.cin != s0.channels || cv.cout != d.channels)
          return bad_op(p, i, "slot shape does not match rulebook / weight");
        if (!rb.nbr || !cv.W) return bad_op(p, i, "null rulebook / weight pointer");
      } else if (op.kind == GPN_NET_BN) {
        if (op.param < 0 || op.param >= p.n_bns) return bad_op(p, i, "table index out of range");
        if (bns[op.param].C != s0.channels || d.channels != s0.channels || d.rows != s0.rows) return bad_op(p, i, "slot shape does not match BatchNorm");
        if (op.src1 >= 0 && (slots[op.src1].rows != s0.rows || slots[op.src1].channels != s0.channels)) return bad_op(p, i, "residual shape");
      } else if (op.kind == GPN_NET_CONCAT) {
        if (op.src1 < 0) return bad_op(p, i, "concat needs two inputs");
        const gpn_net_slot_t& s1 = slots[op.src1];
        if (s1.rows != s0.rows || d.rows != s0.rows || d.channels != s0.channels + s1.channels || s0.channels % 4 || s1.channels % 4)
          return bad_op(p, i, "concat shapes");
      } else {
        return bad_op(p, i, "unknown op kind");
      }
    }
  }
  return GPN_OK;
}

// a BatchNorm over running statistics needs all four vectors, folded into a conv launch (whose epilogue reads them) or not
int check_eval_bn(const Program& p, int i) {
  for (int t = 0; t < p.n_nets; ++t) {
    const gpn_net_bn_t& bn = p.nets[t].bns[p.ops[i].param];
    if (!bn.weight || !bn.bias || !bn.running_mean || !bn.running_var)
      return bad_op(p, i, "BatchNorm needs weight, bias, running_mean and running_var (null pointer)");
  }
  return GPN_OK;
}

// a forward pass: the mode, the tables, every activation pointer; then the workspace
int validate_forward(const Program& p, int mode, void* ws, size_t ws_bytes, Layout& lay) {
  if (mode != 0 && mode != 1 && mode != GPN_NET_INFERENCE) {
    gpn::set_error("%s: training must be 0, 1 or GPN_NET_INFERENCE", p.who);
    return GPN_ERR_ARG;
  }
  int rc = check_program(p);
  for (int i = 0; i < p.n_ops && rc == GPN_OK; ++i) {
    const gpn_net_op_t& op = p.ops[i];
    for (int t = 0; t < p.n_nets; ++t) {
      const gpn_net_slot_t* s = p.nets[t].slots;
      if (!s[op.src0].data || !s[op.dst].data || (op.src1 >= 0 && !s[op.src1].data)) return bad_op(p, i, "null activation pointer");
    }
    if (op.kind == GPN_NET_BN && mode != 1) rc = check_eval_bn(p, i);
  }
  return rc ? rc : layout_of(p, false, ws, ws_bytes, lay);
}

// The pointer checks of a backward pass depend on which slots hold a gradient when the reverse walk reaches an op (an op whose
// output holds none is skipped): a dry walk over a copy of the grad_states, making exactly the transitions the pass will make.
int validate_backward(const Program& p, int need_input_grad, void* ws, size_t ws_bytes, Layout& lay) {
  int rc = check_program(p);
  if (rc) return rc;
  std::vector<int> state[2];
  for (int t = 0; t < p.n_nets; ++t)
    for (int s = 0; s < p.n_slots; ++s) state[t].push_back(p.nets[t].slots[s].grad_state);
  for (int i = p.n_ops - 1; i >= 0; --i) {
    const gpn_net_op_t& op = p.ops[i];
    if (!state[0][op.dst]) continue;  // nothing flows back through this op (its output does not reach the loss)
    const bool to_src0 = op.kind != GPN_NET_CONV || op.src0 != 0 || need_input_grad;  // a gradient is written to src0 ...
    const bool to_src1 =  // ... and to src1
        op.kind == GPN_NET_CONCAT || (op.kind == GPN_NET_BN && op.src1 >= 0 && (op.src1 != 0 || need_input_grad));
    for (int t = 0; t < p.n_nets; ++t) {
      const gpn_net_slot_t* s = p.nets[t].slots;
      if (!s[op.dst].grad || !s[op.src0].data || !s[op.dst].data || state[t][op.dst] != state[0][op.dst])
        return bad_op(p, i, "null pointer (or the two networks' gradient states differ)");
      if (op.kind == GPN_NET_CONV) {
        const gpn_net_rulebook_t& rb = p.rbs[op.rulebook];
        if (p.nets[t].convs[op.param].dW && (!rb.pair_src || !rb.pair_dst || !rb.tile_off)) return bad_op(p, i, "rulebook has no pair lists for wgrad");
        if (to_src0 && (!s[op.src0].grad || !rb.nbr_t)) return bad_op(p, i, "null gradient buffer / transposed table");
      } else if (op.kind == GPN_NET_BN) {
        const gpn_net_bn_t& bn = p.nets[t].bns[op.param];
        if (!s[op.src0].grad || !bn.dweight || !bn.dbias) return bad_op(p, i, "null gradient buffer");
        if (state[t][op.src0]) return bad_op(p, i, "BatchNorm input consumed twice is not supported");
        if (to_src1 && !s[op.src1].grad) return bad_op(p, i, "null residual gradient buffer");
      } else if (!s[op.src0].grad || !s[op.src1].grad) {
        return bad_op(p, i, "null gradient buffer");
      }
    }
    for (int t = 0; t < p.n_nets; ++t) {
      if (to_src0) state[t][op.src0] = 1;
      if (to_src1) state[t][op.src1] = 1;
    }
  }
  return layout_of(p, true, ws, ws_bytes, lay);
}

// ---- the bf16 inference pass: what it holds in its workspace - the packed bf16 weights and ONE bf16 buffer per slot that is materialised - and which
// BatchNorms ride in the conv before them.  A function of the tables alone: gpn_net_forward_bf16_ws_bytes and the pass share it.
struct Bf16Plan {
  std::vector<char> folded;        // BN op i is applied by CONV op i - 1 (whose own output slot is never materialised)
  std::vector<size_t> slot_off;    // by slot: byte offset of its bf16 buffer, kNoBuffer = none
  std::vector<size_t> packed_off;  // by CONV op: byte offset of its packed weight
  int out_slot = -1;               // the slot that is written and never read: receives fp32
  size_t total = 0;
};

int plan_bf16(const char* who, const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, int n_slots,
              const gpn_net_rulebook_t* rbs, const gpn_net_conv_t* convs, Bf16Plan& plan) {
  bool slot0_bf16 = false;  // slot 0 has a reader other than a BatchNorm's input
  for (int i = 0; i < n_ops; ++i) {
    const gpn_net_op_t& op = ops[i];
    if (op.src0 < 0 || op.src0 >= n_slots || op.dst < 0 || op.dst >= n_slots || op.src1 >= n_slots) {
      gpn::set_error("%s: op %d: slot index out of range", who, i);
      return GPN_ERR_ARG;
    }
    if ((op.src0 == 0 && op.kind != GPN_NET_BN) || op.src1 == 0) slot0_bf16 = true;
  }
  const Analysis a = analyse(ops, n_ops, n_slots);
  plan.folded.assign(n_ops, 0);
  for (int i = 0; i < n_ops; ++i)
    if (bn_follows_conv(ops, n_ops, i, a) && !fold_aliases(ops[i], ops[i + 1])) plan.folded[i + 1] = 1;
  std::vector<int> written(n_slots, 0);
  for (int i = 0; i < n_ops; ++i)
    if (!(ops[i].kind == GPN_NET_CONV && i + 1 < n_ops && plan.folded[i + 1])) written[ops[i].dst]++;
  plan.out_slot = -1;
  for (int s = 1; s < n_slots; ++s) {
    if (written[s] > 1) {
      gpn::set_error("%s: slot %d is written by more than one op", who, s);
      return GPN_ERR_ARG;
    }
    if (written[s] && a.readers[s] == 0) {
      if (plan.out_slot >= 0) {
        gpn::set_error("%s: slots %d and %d are both written and never read: the program needs exactly one output slot", who,
                       plan.out_slot, s);
        return GPN_ERR_ARG;
      }
      plan.out_slot = s;
    }
  }
  if (plan.out_slot < 0) {
    gpn::set_error("%s: the program has no output slot (one that is written and never read)", who);
    return GPN_ERR_ARG;
  }
  size_t off = 0;
  plan.packed_off.assign(n_ops, kNoBuffer);
  for (int i = 0; i < n_ops; ++i) {
    if (ops[i].kind != GPN_NET_CONV) continue;
    const gpn_net_conv_t& cv = convs[ops[i].param];
    plan.packed_off[i] = off;
    off += gpn::align_up((size_t)rbs[ops[i].rulebook].K * cv.cin * cv.cout * sizeof(uint16_t));
  }
  plan.slot_off.assign(n_slots, kNoBuffer);
  for (int s = 0; s < n_slots; ++s) {
    if (s == 0 ? !slot0_bf16 : (!written[s] || s == plan.out_slot)) continue;
    plan.slot_off[s] = off;
    off += gpn::align_up((size_t)slots[s].rows * slots[s].channels * sizeof(uint16_t));
  }
  plan.total = off;
  return GPN_OK;
}
}  // namespace
