// net.hip — kernel family U: layer-program executor for the sparse residual U-Net (include/gpn.h section U).
// Reference behaviour: network/backbone.py:40-49 (ResBlock.forward), :126-141 (UBlock.forward), :150-155 (SparseUNet.forward) — a
// Python walk over ~200 spconv / BatchNorm modules per forward, and autograd's walk back.  Here the host describes that walk once
// as a flat list of CONV / BN / CONCAT ops over numbered activation slots and this file issues every launch of the forward (or of
// the backward, in reverse program order) from one native loop.  The arithmetic is exactly that of the per-layer entry points
// (gpn_spconv_fwd_w, gpn_spconv_wgrad, gpn_bn_*), which this file calls; the kernels of its own are the column concat / split, the
// gradient accumulation and a batched weight packer.  In backward the weight-gradient contractions run on a second (lower-priority)
// stream (net_wgrad.h): nothing in the pass consumes dW, so they fill the CUs the dependent dgrad / BN chain of the small, deep
// levels leaves idle.  BatchNorm sums ride in the conv / dgrad epilogues (bn_stats.h), and two structurally identical networks over
// the same rulebooks run as PAIRED passes - one launch per layer for both (NetSet).
// A pass is PLAN (net_plan.h, host only: every table validated, BatchNorms assigned to conv launches, the workspace laid out;
// every argument error is reported there), then EMIT (this file: one function per op kind and direction issues the launches;
// after the first launch only launch errors and the weight-gradient worker's errors remain).
#include <atomic>
#include <string>
#include <vector>

#include "gpn_common.h"
#include "net_plan.h"
#include "net_wgrad.h"
#include "spconv_pack.h"

namespace {
constexpr int kThreads = 256;

// BatchNorm in the conv launches - training: the sums in the conv / dgrad epilogues (bn_stats.h); inference: the whole BatchNorm
// (gpn::ConvAffine) - on / off: gpn_net_bn_fusion(0) restores the separate launches (A/B measurements, and the tests that compare
// the two forms).  (No lambdas in namespace-scope initialisers here: hipcc numbers them per anonymous-namespace block, so one in a
// second block gets the mangled name - and, at link time, the body - of the first block's.)
std::atomic<int> g_bn_fusion{1};

// dst[r, 0:ca] = a[r, :], dst[r, ca:ca+cb] = b[r, :]   (float4 granularity; channel counts are multiples of 4).  Two pointer
// sets per launch, picked by blockIdx.y (paired passes, see NetSet)
struct ConcatPtrs {
  const float4* a;
  const float4* b;
  float4* dst;
};
__global__ __launch_bounds__(kThreads) void concat_kernel(ConcatPtrs pa, ConcatPtrs pb, int64_t rows, int ca4, int cb4,
                                                          const int64_t* __restrict__ rows_dev) {
  rows = gpn::live_rows(rows_dev, rows);
  const ConcatPtrs& p = blockIdx.y ? pb : pa;
  const float4* __restrict__ a = p.a;
  const float4* __restrict__ b = p.b;
  float4* __restrict__ dst = p.dst;
  const int c4 = ca4 + cb4;
  const int64_t total = rows * c4;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / c4;
    const int c = (int)(i - r * c4);
    dst[i] = c < ca4 ? a[r * ca4 + c] : b[r * cb4 + (c - ca4)];
  }
}

// the transpose: da (+)= dsrc[:, 0:ca], db (+)= dsrc[:, ca:]; acc_a / acc_b select overwrite (0) or accumulate (1)
struct SplitPtrs {
  const float4* dsrc;
  float4* da;
  float4* db;
};
__global__ __launch_bounds__(kThreads) void split_kernel(SplitPtrs pa, SplitPtrs pb, int64_t rows, int ca4, int cb4, int acc_a,
                                                         int acc_b, const int64_t* __restrict__ rows_dev) {
  rows = gpn::live_rows(rows_dev, rows);
  const SplitPtrs& pp = blockIdx.y ? pb : pa;
  const float4* __restrict__ dsrc = pp.dsrc;
  float4* __restrict__ da = pp.da;
  float4* __restrict__ db = pp.db;
  const int c4 = ca4 + cb4;
  const int64_t total = rows * c4;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / c4;
    const int c = (int)(i - r * c4);
    const float4 g = dsrc[i];
    float4* p = c < ca4 ? da + (r * ca4 + c) : db + (r * cb4 + (c - ca4));
    if (c < ca4 ? acc_a : acc_b) {
      float4 o = *p;
      o.x += g.x, o.y += g.y, o.z += g.z, o.w += g.w;
      *p = o;
    } else {
      *p = g;
    }
  }
}

__global__ __launch_bounds__(kThreads) void accumulate_kernel(float4* __restrict__ dst, const float4* __restrict__ src,
                                                              int64_t total4, int c4, const int64_t* __restrict__ rows_dev) {
  if (rows_dev) total4 = gpn::live_rows(rows_dev, total4 / c4) * c4;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total4; i += (int64_t)gridDim.x * kThreads) {
    float4 o = dst[i];
    const float4 g = src[i];
    o.x += g.x, o.y += g.y, o.z += g.z, o.w += g.w;
    dst[i] = o;
  }
}

// batched weight packing: up to kPackBatch weights per launch, descriptors passed by value in the kernel arguments
constexpr int kPackBatch = 24;
struct PackDesc {
  const float* W;
  float* packed;
  int K, cin_w, cout_w, flags;
};
struct PackBatch {
  PackDesc d[kPackBatch];
};
__global__ __launch_bounds__(kThreads) void pack_many_kernel(PackBatch batch) {
  const PackDesc d = batch.d[blockIdx.y];
  const int64_t total = (int64_t)d.K * d.cin_w * d.cout_w;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads)
    d.packed[t] = gpn::packed_weight_element(d.W, d.K, d.cin_w, d.cout_w, d.flags, t);
}

inline int grid_for(int64_t total) {
  int64_t g = gpn::cdiv(total, kThreads);
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// the second stream (and the events that order it against the caller's stream), one set per device
constexpr int kForkEvents = 64;
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork[kForkEvents] = {};
  hipEvent_t join = nullptr;
  int next = 0;
};
SideStream* side_stream() {
  static SideStream per_device[gpn::kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= gpn::kMaxDevices) return nullptr;
  SideStream& s = per_device[dev];
  if (!s.stream) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = numerically largest = lowest priority
    // (confining this stream to a subset of the CUs changed nothing at >= 128 CUs and cost 20 % at 64: profiles/r04_cu_mask.txt)
    if (hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking, lo) != hipSuccess) return nullptr;
    for (auto& e : s.fork)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&s.join, hipEventDisableTiming) != hipSuccess) return nullptr;
  }
  return &s;
}

// What the emit functions of a pass share: the tables, the plan of the pass's direction, the workspace layout, the stream(s).
struct Pass {
  const Program& p;
  const Layout& lay;
  hipStream_t stream;
  int mode;  // forward: 0 / 1 / GPN_NET_INFERENCE (see plan_forward); backward: != 0 = the forward pass used batch statistics
  int need_input_grad = 0;
  const FwdPlan* fwd = nullptr;
  const BwdPlan* bwd = nullptr;
  std::vector<const float*> packed_of[2];  // by network and CONV op: its packed weight
  SideStream* side = nullptr;              // (this and the rest: backward only)
  WgradWorker* worker = nullptr;
  bool forked = false;          // a weight-gradient job was published: the caller's stream joins the second one at the end
  std::vector<char> sums_done;  // by BN op: a dgrad launch of this pass has accumulated its backward sums
};

// The start of every pass: the weight of every CONV op is packed into its network's area (transposed [+ tap-reversed] for the
// backward pass; ceil(n_conv / kPackBatch) launches per network), then the BatchNorm sum slabs in use are zeroed.
int pack_and_clear(Pass& c, size_t slab_bytes) {
  const Program& p = c.p;
  for (int t = 0; t < p.n_nets; ++t) {
    c.packed_of[t].assign(p.n_ops, nullptr);
    PackBatch batch;
    int fill = 0;
    int64_t max_total = 0;
    char* dst = c.lay.packed(t);
    for (int i = 0; i < p.n_ops; ++i) {
      if (p.ops[i].kind == GPN_NET_CONV) {
        const gpn_net_rulebook_t& rb = p.rbs[p.ops[i].rulebook];
        const gpn_net_conv_t& cv = p.nets[t].convs[p.ops[i].param];
        const int64_t total = (int64_t)rb.K * cv.cin * cv.cout;
        int flags = GPN_LAYOUT_OKI;
        if (c.lay.backward) flags |= GPN_PACK_TRANSPOSE | (rb.reverse_taps ? GPN_PACK_REVERSE : 0);
        c.packed_of[t][i] = reinterpret_cast<float*>(dst);
        batch.d[fill++] = PackDesc{cv.W, reinterpret_cast<float*>(dst), rb.K, cv.cin, cv.cout, flags};
        max_total = std::max(max_total, total);
        dst += gpn::align_up((size_t)total * sizeof(float));
      }
      if (fill == kPackBatch || (fill && i + 1 == p.n_ops)) {
        const int gx = (int)std::min<int64_t>(gpn::cdiv(max_total, kThreads), 256);
        hipLaunchKernelGGL(pack_many_kernel, dim3(gx, fill), dim3(kThreads), 0, c.stream, batch);
        GPN_CHECK_LAUNCH();
        fill = 0, max_total = 0;
      }
    }
  }
  if (slab_bytes)
    for (int t = 0; t < p.n_nets; ++t) GPN_CHECK_HIP(hipMemsetAsync(c.lay.stats(t), 0, slab_bytes, c.stream));
  return GPN_OK;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
int fwd_conv(const Pass& c, int i) {
  const Program& p = c.p;
  const gpn_net_op_t& op = p.ops[i];
  const gpn_net_rulebook_t& rb = p.rbs[op.rulebook];
  const gpn_net_conv_t& cv = p.nets[0].convs[op.param];
  const gpn_net_slot_t& d = p.nets[0].slots[op.dst];
  // a folded BatchNorm behind this conv: the launch applies it and writes into THAT op's output slot
  const gpn_net_op_t* bo = i + 1 < p.n_ops && c.fwd->folded[i + 1] ? &p.ops[i + 1] : nullptr;
  gpn::ConvStats st;
  st.slot_mask = gpn::stat_slot_count(plan_of(d)) - 1;
  for (int t = 0; t < p.n_nets; ++t) {
    const gpn_net_slot_t* s = p.nets[t].slots;
    gpn::ConvAffine ep;
    if (bo) {
      const gpn_net_bn_t& bn = p.nets[t].bns[bo->param];
      ep.mean = bn.running_mean, ep.var = bn.running_var, ep.weight = bn.weight, ep.bias = bn.bias;
      ep.res = bo->src1 >= 0 ? s[bo->src1].data : nullptr;
      ep.eps = bn.eps, ep.relu = (bo->flags & GPN_NET_RELU) ? 1 : 0;
    }
    if (t == 0) {
      st.slab = c.lay.slab(0, c.fwd->slab[i]), st.ep = ep;
    } else {
      st.twin.in = s[op.src0].data, st.twin.packed = c.packed_of[1][i], st.twin.out = s[bo ? bo->dst : op.dst].data;
      st.twin.slab = c.lay.slab(1, c.fwd->slab[i]), st.twin.ep = ep;
    }
  }
  return gpn::spconv_fwd_into(p.nets[0].slots[op.src0].data, c.packed_of[0][i], rb.nbr, rb.nbr_p, rb.perm, rb.K, rb.n_dst, cv.cin,
                              cv.cout, p.nets[0].slots[bo ? bo->dst : op.dst].data, 0, st, c.lay.op_ws(), c.lay.op_ws_bytes(), c.stream,
                              dev_rows(d));
}

int fwd_bn(const Pass& c, int i) {
  const Program& p = c.p;
  const gpn_net_op_t& op = p.ops[i];
  const gpn_net_slot_t& s0 = p.nets[0].slots[op.src0];
  const int relu = (op.flags & GPN_NET_RELU) ? 1 : 0;
  const bool training = c.mode == 1;
  gpn::BnFwdPtrs pp[2];
  for (int t = 0; t < p.n_nets; ++t) {
    const gpn_net_bn_t& bn = p.nets[t].bns[op.param];
    pp[t].x = p.nets[t].slots[op.src0].data;
    pp[t].res = op.src1 >= 0 ? p.nets[t].slots[op.src1].data : nullptr;
    pp[t].partial = c.lay.slab(t, c.fwd->slab[i]);
    pp[t].weight = bn.weight, pp[t].bias = bn.bias, pp[t].y = p.nets[t].slots[op.dst].data;
    pp[t].mean = bn.save_mean, pp[t].invstd = bn.save_invstd;
    pp[t].running_mean = bn.running_mean, pp[t].running_var = bn.running_var;
  }
  // a pair's two BatchNorms share a launch where the kernel takes a twin (apply pass over a conv's sums; running statistics)
  const gpn_net_bn_t &bn0 = p.nets[0].bns[op.param], &bn1 = p.nets[p.n_nets - 1].bns[op.param];
  const bool shared = p.n_nets == 2 && (!training || pp[0].partial) && bn1.eps == bn0.eps && bn1.momentum == bn0.momentum;
  const gpn::BnFwdPtrs* twin = shared ? &pp[1] : nullptr;
  int rc = GPN_OK;
  for (int t = 0; t < (shared ? 1 : p.n_nets) && rc == GPN_OK; ++t) {
    const gpn_net_bn_t& bn = p.nets[t].bns[op.param];
    if (!training)
      rc = gpn::bn_fwd_eval_running(pp[t], twin, s0.rows, dev_rows(s0), bn.C, bn.eps, relu, c.stream);
    else if (pp[t].partial)
      rc = gpn::bn_fwd_train_fused(pp[t], twin, s0.rows, bn.C, bn.eps, bn.momentum, relu, c.stream, dev_rows(s0));
    else
      rc = gpn::bn_fwd_train_rows(pp[t].x, pp[t].res, bn.weight, bn.bias, s0.rows, dev_rows(s0), bn.C, bn.eps, bn.momentum, relu, pp[t].y,
                                  bn.save_mean, bn.save_invstd, bn.running_mean, bn.running_var, c.lay.op_ws(), c.lay.op_ws_bytes(), c.stream);
  }
  return rc;
}

int fwd_concat(const Pass& c, int i) {
  const gpn_net_op_t& op = c.p.ops[i];
  const gpn_net_slot_t *s = c.p.nets[0].slots, *s2 = c.p.nets[c.p.n_nets - 1].slots;  // (one network: the same set twice)
  const ConcatPtrs pa{(const float4*)s[op.src0].data, (const float4*)s[op.src1].data, (float4*)s[op.dst].data};
  const ConcatPtrs pb{(const float4*)s2[op.src0].data, (const float4*)s2[op.src1].data, (float4*)s2[op.dst].data};
  const gpn_net_slot_t& d = s[op.dst];
  hipLaunchKernelGGL(concat_kernel, dim3(grid_for(plan_of(d) * (d.channels / 4)), c.p.n_nets), dim3(kThreads), 0, c.stream, pa, pb,
                     d.rows, s[op.src0].channels / 4, s[op.src1].channels / 4, d.rows_dev);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

int net_forward_impl(const Program& p, int mode, void* ws, size_t ws_bytes, hipStream_t stream) {
  Layout lay;
  int rc = validate_forward(p, mode, ws, ws_bytes, lay);
  if (rc) return rc;
  const FwdPlan plan = plan_forward(p, mode, g_bn_fusion.load(std::memory_order_relaxed) != 0);
  Pass c{p, lay, stream, mode};
  c.fwd = &plan;
  rc = pack_and_clear(c, plan.slab_bytes);
  for (int i = 0; i < p.n_ops && rc == GPN_OK; ++i) {
    if (plan.folded[i]) continue;  // (applied by the conv before it)
    rc = p.ops[i].kind == GPN_NET_CONV ? fwd_conv(c, i) : p.ops[i].kind == GPN_NET_BN ? fwd_bn(c, i) : fwd_concat(c, i);
  }
  return rc;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// A producer that cannot add in place writes a slot's gradient to the slot's own buffer if nothing was written there yet, else
// to the staging buffer; commit() then adds a staged gradient to the slot's.
inline float* grad_target(const gpn_net_slot_t& s, float* staging) { return s.grad_state ? staging : s.grad; }
int commit(gpn_net_slot_t& s, const float* written, hipStream_t stream) {
  if (written != s.grad) {
    const int64_t total4 = s.rows * s.channels / 4;
    hipLaunchKernelGGL(accumulate_kernel, dim3(grid_for(plan_of(s) * s.channels / 4)), dim3(kThreads), 0, stream, (float4*)s.grad,
                       (const float4*)written, total4, s.channels / 4, s.rows_dev);
    GPN_CHECK_LAUNCH();
  }
  s.grad_state = 1;
  return GPN_OK;
}

// CONV: the weight-gradient contraction forks to the second stream; the dgrad launch stays on the main chain
int bwd_conv(Pass& c, int i) {
  const Program& p = c.p;
  const gpn_net_op_t& op = p.ops[i];
  const gpn_net_rulebook_t& rb = p.rbs[op.rulebook];
  const gpn_net_conv_t& cv = p.nets[0].convs[op.param];
  gpn_net_slot_t &s0 = p.nets[0].slots[op.src0], &d = p.nets[0].slots[op.dst];
  float* dW[2] = {cv.dW, p.n_nets == 2 ? p.nets[1].convs[op.param].dW : nullptr};
  if (dW[0] || dW[1]) {
    // d.grad is final here (every consumer of slot d ran earlier in this reverse walk): fork the contraction
    hipEvent_t ev = c.side->fork[c.side->next];
    c.side->next = (c.side->next + 1) % kForkEvents;
    GPN_CHECK_HIP(hipEventRecord(ev, c.stream));
    auto job = [&](int t, int twin) {  // network t's layer, with network `twin`'s in the same launch (or -1)
      const gpn_net_slot_t *s = p.nets[t].slots, *s2 = twin < 0 ? nullptr : p.nets[twin].slots;
      return WgradJob{s[op.src0].data, s[op.dst].grad, rb.pair_src, rb.pair_dst, rb.tile_off, rb.K, rb.n_dst, dev_rows(d), cv.cin, cv.cout,
                      dW[t], ev, s2 ? s2[op.src0].data : nullptr, s2 ? s2[op.dst].grad : nullptr, s2 ? dW[twin] : nullptr};
    };
    if (dW[0] && dW[1]) {
      c.worker->push(job(0, 1));
    } else {
      for (int t = 0; t < p.n_nets; ++t)
        if (dW[t]) c.worker->push(job(t, -1));
    }
    c.forked = true;
  }
  if (op.src0 == 0 && !c.need_input_grad) return GPN_OK;
  // a slot that already holds a gradient takes this one added in place (no staging buffer, no accumulate launch)
  const int j = c.bwd->fused_by[i];  // the BatchNorm whose backward sums this launch adds, or -1
  gpn::ConvStats st;
  if (j >= 0) {
    st.slot_mask = gpn::stat_slot_count(plan_of(s0)) - 1;
    st.relu = (p.ops[j].flags & GPN_NET_RELU) ? 1 : 0;
    c.sums_done[j] = 1;
  }
  for (int t = 0; t < p.n_nets; ++t) {
    const gpn_net_slot_t* s = p.nets[t].slots;
    unsigned long long* slab = nullptr;
    const float *x = nullptr, *y = nullptr, *mean = nullptr, *invstd = nullptr;
    if (j >= 0) {
      const gpn_net_bn_t& bn = p.nets[t].bns[p.ops[j].param];
      slab = c.lay.slab(t, c.bwd->slab[j]);
      x = s[p.ops[j].src0].data, y = s[op.src0].data;
      mean = c.mode ? bn.save_mean : bn.running_mean, invstd = bn.save_invstd;
    }
    if (t == 0) {
      st.slab = slab, st.x = x, st.y = y, st.mean = mean, st.invstd = invstd;
    } else {
      st.twin.in = s[op.dst].grad, st.twin.packed = c.packed_of[1][i], st.twin.out = s[op.src0].grad;
      st.twin.slab = slab, st.twin.x = x, st.twin.y = y, st.twin.mean = mean, st.twin.invstd = invstd;
    }
  }
  const int rc = gpn::spconv_fwd_into(d.grad, c.packed_of[0][i], rb.nbr_t, rb.nbr_t_p, rb.perm_t, rb.K, rb.n_src, cv.cout, cv.cin, s0.grad,
                                      s0.grad_state ? 1 : 0, st, c.lay.op_ws(), c.lay.op_ws_bytes(), c.stream, dev_rows(s0));
  for (int t = 0; t < p.n_nets && rc == GPN_OK; ++t) p.nets[t].slots[op.src0].grad_state = 1;
  return rc;
}

int bwd_bn(Pass& c, int i) {
  const Program& p = c.p;
  const gpn_net_op_t& op = p.ops[i];
  const gpn_net_slot_t& s0 = p.nets[0].slots[op.src0];
  const int relu = (op.flags & GPN_NET_RELU) ? 1 : 0;
  const int training = c.mode ? 1 : 0;
  gpn::BnBwdPtrs pp[2];
  for (int t = 0; t < p.n_nets; ++t) {
    const gpn_net_bn_t& bn = p.nets[t].bns[op.param];
    const gpn_net_slot_t* s = p.nets[t].slots;
    pp[t].x = s[op.src0].data, pp[t].y = s[op.dst].data, pp[t].dy = s[op.dst].grad;
    pp[t].partial = c.lay.slab(t, c.bwd->slab[i]);
    pp[t].mean = training ? bn.save_mean : bn.running_mean;
    pp[t].invstd = bn.save_invstd, pp[t].weight = bn.weight;
    pp[t].dx = s[op.src0].grad;  // (validation has refused a BatchNorm input that already holds a gradient)
    if (op.src1 >= 0 && (op.src1 != 0 || c.need_input_grad)) pp[t].dres = grad_target(s[op.src1], c.lay.staging(t));
    pp[t].dweight = bn.dweight, pp[t].dbias = bn.dbias;
  }
  const int C = p.nets[0].bns[op.param].C;
  const bool shared = c.sums_done[i] && p.n_nets == 2;  // the apply pass over sums from a dgrad launch takes a twin
  int rc = GPN_OK;
  for (int t = 0; t < (shared ? 1 : p.n_nets) && rc == GPN_OK; ++t) {
    if (c.sums_done[i])
      rc = gpn::bn_bwd_fused(pp[t], shared ? &pp[1] : nullptr, s0.rows, C, relu, training, c.stream, dev_rows(s0));
    else
      rc = gpn::bn_bwd_rows(pp[t].x, pp[t].y, pp[t].dy, pp[t].weight, pp[t].mean, pp[t].invstd, s0.rows, dev_rows(s0), C, relu, training,
                            pp[t].dx, pp[t].dres, pp[t].dweight, pp[t].dbias, c.lay.op_ws(), c.lay.op_ws_bytes(), c.stream);
  }
  for (int t = 0; t < p.n_nets && rc == GPN_OK; ++t) {
    p.nets[t].slots[op.src0].grad_state = 1;
    if (pp[t].dres) rc = commit(p.nets[t].slots[op.src1], pp[t].dres, c.stream);
  }
  return rc;
}

int bwd_split(Pass& c, int i) {
  const gpn_net_op_t& op = c.p.ops[i];
  const gpn_net_slot_t *s = c.p.nets[0].slots, *s2 = c.p.nets[c.p.n_nets - 1].slots;  // (one network: the same set twice)
  const SplitPtrs pa{(const float4*)s[op.dst].grad, (float4*)s[op.src0].grad, (float4*)s[op.src1].grad};
  const SplitPtrs pb{(const float4*)s2[op.dst].grad, (float4*)s2[op.src0].grad, (float4*)s2[op.src1].grad};
  const gpn_net_slot_t& d = s[op.dst];
  hipLaunchKernelGGL(split_kernel, dim3(grid_for(plan_of(d) * (d.channels / 4)), c.p.n_nets), dim3(kThreads), 0, c.stream, pa, pb, d.rows,
                     s[op.src0].channels / 4, s[op.src1].channels / 4, s[op.src0].grad_state, s[op.src1].grad_state, d.rows_dev);
  GPN_CHECK_LAUNCH();
  for (int t = 0; t < c.p.n_nets; ++t) c.p.nets[t].slots[op.src0].grad_state = c.p.nets[t].slots[op.src1].grad_state = 1;
  return GPN_OK;
}

int net_backward_impl(const Program& p, int training, int need_input_grad, void* ws, size_t ws_bytes, hipStream_t stream) {
  Layout lay;
  int rc = validate_backward(p, need_input_grad, ws, ws_bytes, lay);
  if (rc) return rc;
  const BwdPlan plan = plan_backward(p, need_input_grad, g_bn_fusion.load(std::memory_order_relaxed) != 0);
  Pass c{p, lay, stream, training, need_input_grad};
  c.bwd = &plan;
  c.sums_done.assign(p.n_ops, 0);
  int device = 0;
  c.side = side_stream();  // (nullptr also for a device ordinal beyond kMaxDevices)
  if (!c.side || hipGetDevice(&device) != hipSuccess) {
    gpn::set_error("%s: could not create the weight-gradient stream", p.who);
    return GPN_ERR_HIP;
  }
  rc = pack_and_clear(c, plan.slab_bytes);
  if (rc) return rc;
  // the side stream may still be reading the workspace of the previous call on this device
  GPN_CHECK_HIP(hipEventRecord(c.side->join, c.side->stream));
  GPN_CHECK_HIP(hipStreamWaitEvent(stream, c.side->join, 0));
  DeviceWorker& dw = device_worker(device);
  std::lock_guard<std::mutex> pass_lock(dw.pass_mu);
  c.worker = &dw.worker;
  c.worker->begin(device, c.side->stream, lay.wgrad_ws(), lay.wgrad_ws_bytes(), (size_t)p.n_ops * p.n_nets);
  // the reverse walk; however it ends, the pass must be closed, or the worker would spin forever
  for (int i = p.n_ops - 1; i >= 0 && rc == GPN_OK; --i) {
    if (!p.nets[0].slots[p.ops[i].dst].grad_state) continue;  // nothing flows back through this op (its output does not reach the loss)
    rc = p.ops[i].kind == GPN_NET_CONV ? bwd_conv(c, i) : p.ops[i].kind == GPN_NET_BN ? bwd_bn(c, i) : bwd_split(c, i);
  }
  std::string worker_err;
  const int worker_rc = c.worker->finish(worker_err);
  if (rc) return rc;
  if (worker_rc) {
    gpn::set_error("%s", worker_err.c_str());
    return worker_rc;
  }
  if (c.forked) {  // join: whatever the caller enqueues next (optimizer, the next pass) sees every dW
    GPN_CHECK_HIP(hipEventRecord(c.side->join, c.side->stream));
    GPN_CHECK_HIP(hipStreamWaitEvent(stream, c.side->join, 0));
  }
  return GPN_OK;
}
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------
// conv-epilogue BatchNorm sums on (1, default) / off (0); on < 0 queries.  Returns the previous setting.
extern "C" int gpn_net_bn_fusion(int on) {
  return on < 0 ? g_bn_fusion.load(std::memory_order_relaxed) : g_bn_fusion.exchange(on ? 1 : 0, std::memory_order_relaxed);
}

extern "C" int gpn_net_wgrad_group(int layers) {
  if (layers < 1) return g_wgrad_group.load(std::memory_order_relaxed);
  return g_wgrad_group.exchange(layers > gpn::kWgradSets ? gpn::kWgradSets : layers, std::memory_order_relaxed);
}

extern "C" size_t gpn_net_ws_bytes(const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, int /*n_slots*/,
                                   const gpn_net_rulebook_t* rulebooks, const gpn_net_conv_t* convs) {
  if (!ops || !slots) return 0;
  return Layout{workspace_need(ops, n_ops, slots, rulebooks, convs), 1, true, nullptr, 0}.total();
}

extern "C" int gpn_net_forward(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots, const gpn_net_rulebook_t* rbs,
                               int n_rbs, const gpn_net_conv_t* convs, int n_convs, const gpn_net_bn_t* bns, int n_bns, int training,
                               void* ws, size_t ws_bytes, gpn_stream_t stream) {
  const NetSet one{slots, convs, bns};
  const Program p{__func__, ops, n_ops, &one, 1, n_slots, rbs, n_rbs, n_convs, n_bns};
  return net_forward_impl(p, training, ws, ws_bytes, (hipStream_t)stream);
}

// two structurally identical networks over the same rulebooks in one pass (see NetSet); workspace: 2 x gpn_net_ws_bytes
extern "C" int gpn_net_forward_pair(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots_a, gpn_net_slot_t* slots_b, int n_slots,
                                    const gpn_net_rulebook_t* rbs, int n_rbs, const gpn_net_conv_t* convs_a,
                                    const gpn_net_conv_t* convs_b, int n_convs, const gpn_net_bn_t* bns_a, const gpn_net_bn_t* bns_b,
                                    int n_bns, int training, void* ws, size_t ws_bytes, gpn_stream_t stream) {
  const NetSet two[2] = {{slots_a, convs_a, bns_a}, {slots_b, convs_b, bns_b}};
  const Program p{__func__, ops, n_ops, two, 2, n_slots, rbs, n_rbs, n_convs, n_bns};
  return net_forward_impl(p, training, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int gpn_net_backward(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots, const gpn_net_rulebook_t* rbs,
                                int n_rbs, const gpn_net_conv_t* convs, int n_convs, const gpn_net_bn_t* bns, int n_bns, int training,
                                int need_input_grad, void* ws, size_t ws_bytes, gpn_stream_t stream) {
  const NetSet one{slots, convs, bns};
  const Program p{__func__, ops, n_ops, &one, 1, n_slots, rbs, n_rbs, n_convs, n_bns};
  return net_backward_impl(p, training, need_input_grad, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int gpn_net_backward_pair(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots_a, gpn_net_slot_t* slots_b, int n_slots,
                                     const gpn_net_rulebook_t* rbs, int n_rbs, const gpn_net_conv_t* convs_a,
                                     const gpn_net_conv_t* convs_b, int n_convs, const gpn_net_bn_t* bns_a, const gpn_net_bn_t* bns_b,
                                     int n_bns, int training, int need_input_grad, void* ws, size_t ws_bytes, gpn_stream_t stream) {
  const NetSet two[2] = {{slots_a, convs_a, bns_a}, {slots_b, convs_b, bns_b}};
  const Program p{__func__, ops, n_ops, two, 2, n_slots, rbs, n_rbs, n_convs, n_bns};
  return net_backward_impl(p, training, need_input_grad, ws, ws_bytes, (hipStream_t)stream);
}

// ---- the bf16 inference pass (include/gpn.h section C16; kernels in spconv_bf16.hip; its plan: net_plan.h) -------------------
extern "C" size_t gpn_net_forward_bf16_ws_bytes(const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, int n_slots,
                                                const gpn_net_rulebook_t* rulebooks, const gpn_net_conv_t* convs) {
  if (!ops || !slots || n_ops < 1 || n_slots < 1) return 0;
  Bf16Plan plan;
  if (plan_bf16(__func__, ops, n_ops, slots, n_slots, rulebooks, convs, plan) != GPN_OK) return 0;
  return plan.total;
}

extern "C" int gpn_net_forward_bf16(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots,
                                    const gpn_net_rulebook_t* rbs, int n_rbs, const gpn_net_conv_t* convs, int n_convs,
                                    const gpn_net_bn_t* bns, int n_bns, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  const char* who = __func__;
  hipStream_t stream = (hipStream_t)stream_;
  const NetSet one{slots, convs, bns};
  const Program p{who, ops, n_ops, &one, 1, n_slots, rbs, n_rbs, n_convs, n_bns};
  int rc = check_program(p);
  if (rc) return rc;
  // ---- everything is validated before the first launch ----
  for (int s = 0; s < n_slots; ++s)
    if (slots[s].rows_dev) {
      gpn::set_error("%s: slot %d: device-counted row counts (rows_dev) are not supported by the bf16 pass", who, s);
      return GPN_ERR_ARG;
    }
  for (int i = 0; i < n_ops; ++i) {
    const gpn_net_op_t& op = ops[i];
    if (op.kind == GPN_NET_CONV) {
      const gpn_net_rulebook_t& rb = rbs[op.rulebook];
      const gpn_net_conv_t& cv = convs[op.param];
      rc = gpn::spconv_bf16_check(who, rb.K, rb.n_dst, cv.cin, cv.cout);
      if (rc) return rc;
      if ((rb.nbr_p == nullptr) != (rb.perm == nullptr)) {
        gpn::set_error("%s: op %d: a tile order needs both nbr_p and perm", who, i);
        return GPN_ERR_ARG;
      }
    } else if (op.kind == GPN_NET_BN) {
      rc = check_eval_bn(p, i);
      if (rc) return rc;
    }
  }
  if (n_ops < 1) {
    gpn::set_error("%s: empty program", who);
    return GPN_ERR_ARG;
  }
  Bf16Plan plan;
  rc = plan_bf16(who, ops, n_ops, slots, n_slots, rbs, convs, plan);
  if (rc) return rc;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i].kind == GPN_NET_CONCAT && ops[i].dst == plan.out_slot) {
      gpn::set_error("%s: op %d: a concat cannot write the (fp32) output slot", who, i);
      return GPN_ERR_ARG;
    }
  if (!slots[0].data || !slots[plan.out_slot].data) {
    gpn::set_error("%s: null activation pointer (input slot 0 / output slot %d)", who, plan.out_slot);
    return GPN_ERR_ARG;
  }
  if (!ws || ws_bytes < plan.total) {
    gpn::set_error("%s: workspace too small (%zu needed, %zu given)", who, plan.total, ws_bytes);
    return GPN_ERR_WS;
  }
  // ---- launches ----
  char* base = static_cast<char*>(ws);
  auto buf = [&](int s) { return reinterpret_cast<uint16_t*>(base + plan.slot_off[s]); };
  std::vector<gpn::PackBf16Desc> descs;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i].kind == GPN_NET_CONV) {
      const gpn_net_conv_t& cv = convs[ops[i].param];
      descs.push_back(gpn::PackBf16Desc{cv.W, reinterpret_cast<uint16_t*>(base + plan.packed_off[i]), rbs[ops[i].rulebook].K, cv.cin,
                                        cv.cout, 1});
    }
  rc = gpn::pack_bf16_many(descs.data(), (int)descs.size(), stream);
  if (rc) return rc;
  if (plan.slot_off[0] != kNoBuffer) {
    rc = gpn::rows_to_bf16_launch(slots[0].data, slots[0].rows * slots[0].channels, buf(0), stream);
    if (rc) return rc;
  }
  for (int i = 0; i < n_ops; ++i) {
    const gpn_net_op_t& op = ops[i];
    if (plan.folded[i]) continue;  // (applied by the conv before it)
    const gpn_net_slot_t &s0 = slots[op.src0], &d = slots[op.dst];
    if (op.kind == GPN_NET_CONV) {
      const gpn_net_rulebook_t& rb = rbs[op.rulebook];
      const gpn_net_conv_t& cv = convs[op.param];
      gpn_conv_epilogue_bf16_t ep{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, 0};
      int dst = op.dst;
      if (i + 1 < n_ops && plan.folded[i + 1]) {
        const gpn_net_op_t& bo = ops[i + 1];
        const gpn_net_bn_t& bn = bns[bo.param];
        ep.mean = bn.running_mean, ep.var = bn.running_var, ep.weight = bn.weight, ep.bias = bn.bias;
        ep.res = bo.src1 >= 0 ? buf(bo.src1) : nullptr;
        ep.eps = bn.eps, ep.relu = (bo.flags & GPN_NET_RELU) ? 1 : 0;
        dst = bo.dst;
      }
      ep.out_f32 = dst == plan.out_slot ? 1 : 0;
      void* out = ep.out_f32 ? static_cast<void*>(slots[dst].data) : static_cast<void*>(buf(dst));
      rc = gpn::spconv_bf16_launch(buf(op.src0), reinterpret_cast<const uint16_t*>(base + plan.packed_off[i]), rb.nbr, rb.nbr_p,
                                   rb.perm, rb.K, rb.n_dst, cv.cin, cv.cout, &ep, out, stream);
    } else if (op.kind == GPN_NET_BN) {
      const gpn_net_bn_t& bn = bns[op.param];
      const bool from_input = op.src0 == 0;  // the fp32 input itself
      const int out_f32 = op.dst == plan.out_slot ? 1 : 0;
      rc = gpn::bn_act_bf16_launch(from_input ? static_cast<const void*>(s0.data) : static_cast<const void*>(buf(op.src0)),
                                   from_input ? 1 : 0, op.src1 >= 0 ? buf(op.src1) : nullptr, bn.weight, bn.bias, bn.running_mean,
                                   bn.running_var, bn.eps, s0.rows, bn.C, (op.flags & GPN_NET_RELU) ? 1 : 0, out_f32,
                                   out_f32 ? static_cast<void*>(d.data) : static_cast<void*>(buf(op.dst)), stream);
    } else {
      rc = gpn::concat_bf16_launch(buf(op.src0), buf(op.src1), buf(op.dst), d.rows, s0.channels, slots[op.src1].channels, stream);
    }
    if (rc) return rc;
  }
  return GPN_OK;
}
