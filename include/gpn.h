/*
 * gpn.h — C-ABI of libgpn_hip.so: the MI355X (gfx950) implementation of the GAPartNet
 * sparse-3D-conv perception hot path.
 *
 * Boundary contract:
 *   - extern "C", plain pointers and sizes, no torch types.  Every pointer is a DEVICE pointer
 *     unless the parameter name ends in `_host`.
 *   - the caller allocates every output and the workspace (query `*_ws_bytes`); kernels never allocate.
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*).
 *   - return value 0 = ok; otherwise an error code, message via gpn_last_error().  The library never
 *     calls exit() (the vendored reference lib does: ball_query_gpu.cu:62-66) so DDP ranks survive.
 *   - data-dependent sizes are written to a device counter; the caller sizes buffers by the stated
 *     upper bound and reads the counter when it needs the value on the host.
 *
 * Each entry point cites the reference interface it replaces (file:line relative to the
 * PKU-EPIC/GAPartNet tree).
 */
#ifndef GPN_H
#define GPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gpn_stream_t; /* hipStream_t */

#define GPN_OK 0
#define GPN_ERR_ARG 1      /* bad argument (null pointer, unsupported size) */
#define GPN_ERR_WS 2       /* workspace too small */
#define GPN_ERR_HIP 3      /* a HIP runtime call / kernel launch failed */

const char* gpn_last_error(void);
int gpn_version(void);
/* number of exported compute entry points and their names (used by the symbol test) */
int gpn_num_entry_points(void);
const char* gpn_entry_point_name(int i);

/* ---- H: dense heads: y = x W^T + b on [N, cin] rows, cin % 4 == 0, cin, cout <= 64 (csrc/linear.hip) ----------------------
 * Replaces torch.nn.functional.linear of network/model.py:140, 159-160, 322, 337 (sem_seg_head, offset_head, score_head,
 * npcs_head) and its autograd: W [cout, cin] in torch.nn.Linear's layout, b [cout] or NULL.  One launch forward; backward
 * writes dx [N, cin], dW [cout, cin], db [cout] (each may be NULL = skipped), deterministic (fixed-order sums). */
int gpn_linear_supported(int cin, int cout);
int gpn_linear_fwd(const float* x, const float* W, const float* b, int64_t N, int cin, int cout, float* y, gpn_stream_t stream);
size_t gpn_linear_bwd_ws_bytes(int64_t N, int cin, int cout);
int gpn_linear_bwd(const float* x, const float* W, const float* dy, int64_t N, int cin, int cout, float* dx, float* dW, float* db,
                   void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ---- PM: dense point-MLP layers of the PointNet backbone on the fp32 MFMA (csrc/pointmlp.hip) -------------------------------
 * Replaces the Conv1d(k = 1) / Linear layers, the two torch.bmm and the max over points of network/pointnet/pointnet_utils.py
 * and pointnet_sem_seg.py.  Forward, for rows r < N of fp32 data in S contiguous, non-empty segments (offsets [S + 1] i64 on
 * the device; NULL with S == 1 = one segment; offsets_host = the caller's host copy or NULL, checked when given):
 *     Y[r, :] = epi( X~[r, :] . W_s(r)^T + b + G[s(r), :] )
 *   X~  row-major [N, cin] (strided == 0), or the view (segment b, channel c, point n of the segment) -> x[b sb + c sc + n sn]
 *   W   [cout, cin] (per_segment == 0) or [S, cout, cin]; b [cout] and G [S, cout] optional
 *   epi y -> epi_scale[c] y + epi_shift[c] (both or neither), then max(0, .) if relu
 *   Y   [N, cout] or NULL;  M [S, cout] or NULL = per-segment column maxima of the same values (deterministic); one of the
 *       two at least.  With Y == NULL the layer's output is never written.
 * No row tile mixes two segments.  dgrad (dX = dY W_s) is this call on transposed weights.
 * wgrad: dW [cout, cin] (or [S, cout, cin]) = dY^T X~ and db [cout] = column sums of dY (either may be NULL), reduced over
 * fixed row chunks on the MFMA and summed in chunk order: deterministic, no float atomics.
 * 1 <= cin <= 4096, 1 <= cout <= 8192 (gpn_pointmlp_supported); N == 0 is GPN_OK. */
int gpn_pointmlp_supported(int cin, int cout);
int gpn_pointmlp_fwd(const float* x, int strided, int64_t sb, int64_t sc, int64_t sn, const float* W, int per_segment,
                     const float* b, const float* G, const float* epi_scale, const float* epi_shift, int relu,
                     const int64_t* offsets, const int64_t* offsets_host, int64_t S, int64_t N, int cin, int cout, float* Y,
                     float* M, gpn_stream_t stream);
size_t gpn_pointmlp_wgrad_ws_bytes(int64_t N, int64_t S, int cin, int cout);
int gpn_pointmlp_wgrad(const float* x, int strided, int64_t sb, int64_t sc, int64_t sn, const float* dy, const int64_t* offsets,
                       const int64_t* offsets_host, int64_t S, int64_t N, int cin, int cout, int per_segment, float* dW,
                       float* db, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ---- optional in-library kernel timing (hipEvent pairs around launches; used by bench.py) ------- */
/* kernel ids for gpn_prof_get */
enum {
  GPN_K_SPCONV_FWD = 0, /* fused gather-MFMA-scatter conv (forward and dgrad launches) */
  GPN_K_SPCONV_WGRAD = 1,
  GPN_K_VOXELIZE = 2,
  GPN_K_RULEBOOK = 3,
  GPN_K_BALL_QUERY = 4,
  GPN_K_CCL = 5,
  GPN_K_BN = 6, /* BatchNorm passes (statistics where not taken by a conv epilogue, apply forward / backward) */
  GPN_K_LINEAR = 7, /* the dense heads (section H) */
  GPN_K_POINTMLP = 8, /* the PointNet backbone's dense layers (section PM): forward / dgrad and wgrad launches */
  GPN_K_COUNT = 9
};
/* fixed cost of a (start event, launch, stop event) bracket, measured around an empty kernel on `stream` (median, us):
 * subtract it from hipEvent-measured launch durations before comparing them with a profiler's kernel durations. */
int gpn_prof_bracket_overhead_us(gpn_stream_t stream, double* overhead_us);
int gpn_prof_enable(int on);
int gpn_prof_reset(void);
/* synchronises the recorded events; returns launches, total milliseconds, algorithmic flops and bytes */
int gpn_prof_get(int kernel_id, int64_t* launches_host, double* ms_host, double* flops_host,
                 double* bytes_host);
/* the same measurements launch by launch, in launch order (first `cap` records; *count_host = how many there are).  tag of a
 * conv fwd / dgrad launch: bit 62 = two problems in the launch (paired pass), bits 48-53 taps K, 40-47 cin / 16, 32-39
 * cout / 16, 0-31 rows of the launch's output; 0 = untagged. */
int gpn_prof_get_launches(int kernel_id, int64_t cap, double* ms_host, int64_t* tag_host, int64_t* count_host);

/* ================================================================================================
 * V — voxelize.   replaces epic_ops.voxelize.voxelize (call sites dataset/gapartnet.py:188-195,
 * network/grouping_utils.py:93-101).
 *   points [M,3] f32, feats [M,C] f32, seg_offsets [S+1] i64 (CSR over points),
 *   seg_range_min/max [S,3] f32 (per segment; the reference passes one range per call — the
 *   host wrapper broadcasts it), voxel_size_host[3], grid_dims_host[3] = cells per axis used to
 *   linearise keys (points whose cell index >= grid_dims are dropped like out-of-range points).
 *   coord = floor((p - range_min) / voxel_size) evaluated in fp32 without contraction.
 * outputs (capacity M rows each): voxel_feats [V,C] (mean, summed in ascending point order),
 *   voxel_coords [V,3] i32, voxel_seg [V] i32, pc_voxel_id [M] i32 (-1 = dropped),
 *   num_voxels [1] i64.  Voxels are ordered by ascending (segment,x,y,z).
 * ================================================================================================ */
size_t gpn_voxelize_ws_bytes(int64_t M, int C);
int gpn_voxelize(const float* points, const float* feats, const int64_t* seg_offsets,
                 const float* seg_range_min, const float* seg_range_max, int64_t M, int C, int64_t S,
                 const float* voxel_size_host, const int32_t* grid_dims_host, float* voxel_feats,
                 int32_t* voxel_coords, int32_t* voxel_seg, int32_t* pc_voxel_id, int64_t* num_voxels,
                 void* ws, size_t ws_bytes, gpn_stream_t stream);

/* same, plus the CSR of points grouped by voxel: point_order [M] i32 (point ids sorted by voxel,
 * ascending point id inside a voxel; dropped points last) and voxel_point_start [M+1] i32 (first V+1
 * entries valid).  Either may be NULL.  Feeds gpn_scatter_rows_csr (the gather's transpose). */
int gpn_voxelize_ex(const float* points, const float* feats, const int64_t* seg_offsets,
                    const float* seg_range_min, const float* seg_range_max, int64_t M, int C, int64_t S,
                    const float* voxel_size_host, const int32_t* grid_dims_host, float* voxel_feats,
                    int32_t* voxel_coords, int32_t* voxel_seg, int32_t* pc_voxel_id, int64_t* num_voxels,
                    int32_t* point_order, int32_t* voxel_point_start, void* ws, size_t ws_bytes,
                    gpn_stream_t stream);

/* scene batches with the reference's per-scene conventions (dataset/gapartnet.py:179-205: range = [min - 1e-4, max + 1e-4]
 * of each scene, cell = floor((p - range_min) / voxel_size)) WITHOUT a host read before or between the launches: per-scene
 * range reduced on the device, keys packed with 10 bits per axis, and ONE read of `stats` [8 + n_levels] i64 afterwards:
 *   [0] #voxels, [1..3] largest cell index per axis (spatial extent = max(that + 1, 128)), [4] dropped points,
 *   [5] != 0: a cell index >= 1024 occurred (results incomplete: use gpn_voxelize_ex with the true extent),
 *   [8 + l] rows of stride-2 level l + 1 below the voxel set (= gpn_rulebook_level_counts), l < n_levels.
 * indices4 [M,4] i32 = (segment, x, y, z) per voxel; the other outputs as gpn_voxelize_ex; same order, same means. */
/* round 5: gpn_voxelize_scenes runs WITHOUT a sort (BASELINE.json "hash-table voxelization"): cell occupancy in a bitmap laid out in
 * (segment, x, y, z) order over the batch's grid (cells per axis reduced on the device), voxel id = popcount rank of the cell's bit,
 * points grouped by a counting placement + an ascending sort of every voxel's own few points.  Bit-identical outputs.  stats[5] = 2:
 * the batch's grid exceeds the bitmap (2^27 cells) - like stats[5] = 1 (a cell index >= 1024) the caller takes another path:
 * gpn_voxelize_scenes_sorted (the stable radix sort of 10-bit-per-axis packed keys; same contract, same workspace query). */
size_t gpn_voxelize_scenes_ws_bytes(int64_t M, int C, int64_t S, int n_levels);
int gpn_voxelize_scenes_sorted(const float* points, const float* feats, const int64_t* seg_offsets, int64_t M, int C, int64_t S,
                               const float* voxel_size_host, int n_levels, float* voxel_feats, int32_t* indices4,
                               int32_t* pc_voxel_id, int32_t* point_order, int32_t* voxel_point_start, int64_t* stats, void* ws,
                               size_t ws_bytes, gpn_stream_t stream);
int gpn_voxelize_scenes(const float* points, const float* feats, const int64_t* seg_offsets, int64_t M, int C, int64_t S,
                        const float* voxel_size_host, int n_levels, float* voxel_feats, int32_t* indices4,
                        int32_t* pc_voxel_id, int32_t* point_order, int32_t* voxel_point_start, int64_t* stats, void* ws,
                        size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * K1/K2 — rulebooks.   replace the indice-pair construction inside spconv.pytorch.SubMConv3d /
 * SparseConv3d / SparseInverseConv3d (call sites network/backbone.py:19-36,74-90,149-152).
 *
 * A rulebook is a set of K pair lists, stored flat and ordered by (tap k, dst row):
 *   pair_src [P] i32, pair_dst [P] i32, tile_off [K, n_tiles+1] i32 where
 *   tile_off[k][t] = index of the first pair of tap k whose dst >= t*GPN_TILE_ROWS
 *   (so tile_off[k][0] is the start of list k and tile_off[k][n_tiles] its end).
 * Each dst row appears at most once per tap.  n_tiles = ceil(n_dst / GPN_TILE_ROWS).
 * ================================================================================================ */
#define GPN_TILE_ROWS 32

/* SubM k=3 pad=1: indices [N,4] i32 (batch,x,y,z); tap = (dx+1)*9+(dy+1)*3+(dz+1); src = row at
 * coord(dst)+delta.  pair arrays need capacity 27*N.  num_pairs [1] i64.
 * nbr (optional, capacity 27*N+1): the tap-major neighbour table nbr[k*N + dst] = src row or -1 that the fused
 * conv kernel (gpn_spconv_fwd) gathers from; the pair lists are its compaction and feed gpn_spconv_wgrad. */
size_t gpn_rulebook_subm3_ws_bytes(int64_t N);
int gpn_rulebook_subm3(const int32_t* indices, int64_t N, const int32_t* spatial_shape_host, int32_t* nbr,
                       int32_t* pair_src, int32_t* pair_dst, int32_t* tile_off, int64_t* num_pairs,
                       void* ws, size_t ws_bytes, gpn_stream_t stream);

/* tile order for the fused conv (optional, large levels): rows of every block of block_rows (power of two) consecutive
 * rows sorted by their neighbour mask (which of the K <= 32 taps exist), stable.  perm [ceil(n/16)*16 + 16] i32 (padding
 * = n-1), nbr_p [K*n + 1] i32 = nbr with its columns in that order. */
size_t gpn_rulebook_tile_order_ws_bytes(int64_t n);
int gpn_rulebook_tile_order(const int32_t* nbr, int K, int64_t n, int block_rows, int32_t* perm, int32_t* nbr_p,
                            void* ws, size_t ws_bytes, gpn_stream_t stream);
/* k=2 stride=2 down-conv.  out shape = floor(D/2) per axis; inputs mapping outside are dropped.
 * Produces the coarse index set (ascending linear key; capacity N rows), fine_to_coarse [N] i32
 * (-1 = dropped), tap [N] i32 = (x&1)*4+(y&1)*2+(z&1), num_out [1] i64.
 * The two pair-list views (dst = coarse for the down conv / dgrad of the inverse conv;
 * dst = fine for the inverse conv / dgrad of the down conv) are then built with
 * gpn_rulebook_down_lists once num_out is known on the host.
 * Two forms, chosen by the workspace passed in: when an occupancy bitmap of the coarse grid (8 bytes per 64 cells of
 * batch_size * floor(D/2)^3, + 4 bytes per word of prefixes, + 4 bytes per 1024 words) fits ws_bytes, the coarse rows are
 * ranked by popcount prefixes over it (no sort); otherwise the rows' coarse keys are radix-sorted, which needs only the
 * gpn_rulebook_down_ws_bytes(N) bytes.  Both forms give identical outputs (tests/test_gpu_rulebooks.py), so a larger
 * workspace only makes the call faster.  Rows with a batch entry outside [0, batch_size) or a negative coordinate are dropped.
 * gpn_rulebook_down_lists with n_out == 0 (every row dropped) writes all-zero offsets and tables of -1. */
size_t gpn_rulebook_down_ws_bytes(int64_t N);
int gpn_rulebook_down(const int32_t* indices, int64_t N, int64_t batch_size,
                      const int32_t* spatial_shape_host, int32_t* out_indices, int32_t* fine_to_coarse, int32_t* tap, int64_t* num_out,
                      void* ws, size_t ws_bytes, gpn_stream_t stream);
/* the K = 1 rulebook of a SubMConv3d(k=1) (network/backbone.py:19-20, the residual blocks' shortcut) / linear layer over n rows
 * (every row its own neighbour): rows [max(n,1)] (serves as
 * pair_src and pair_dst), tile_off [n_tiles + 1], nbr [n + 1], num_pairs [1] - one launch instead of seven torch ops */
int gpn_rulebook_identity(int64_t n, int32_t* rows, int32_t* tile_off, int32_t* nbr, int64_t* num_pairs, gpn_stream_t stream);
/* row counts of ALL coarse levels below a voxel set in one pass (what n_levels successive gpn_rulebook_down calls - the
 * SparseConv3d(k=2,s=2) of every UBlock, network/backbone.py:74-77 - would report in num_out): counts [n_levels] i64 on the device, so that a U-Net's rulebook pyramid costs ONE host read instead of
 * one per level; gpn_rulebook_down itself is unchanged (its num_out is then only a cross-check).  n_dev (optional, device):
 * the number of valid rows when indices is an upper-bound buffer. */
size_t gpn_rulebook_level_counts_ws_bytes(int64_t n_max, int n_levels);
int gpn_rulebook_level_counts(const int32_t* indices, int64_t n_max, const int64_t* n_dev, int64_t batch_size,
                              const int32_t* spatial_shape_host, int n_levels, int64_t* counts, void* ws, size_t ws_bytes,
                              gpn_stream_t stream);
size_t gpn_rulebook_down_lists_ws_bytes(int64_t N, int64_t n_out);
int gpn_rulebook_down_lists(const int32_t* fine_to_coarse, const int32_t* tap, int64_t N,
                            int64_t n_out,
                            int32_t* fwd_nbr /* [8*n_out+1] or NULL */, int32_t* fwd_src, int32_t* fwd_dst,
                            int32_t* fwd_tile_off, /* dst = coarse, cap N */
                            int32_t* bwd_nbr /* [8*N+1] or NULL */, int32_t* bwd_src, int32_t* bwd_dst,
                            int32_t* bwd_tile_off, /* dst = fine, cap N */
                            int64_t* num_pairs, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * C — sparse convolution.  replaces the conv forward/backward inside spconv (network/backbone.py).
 * weights: canonical layout W [K, Cin, Cout] row-major fp32 (tap-major).
 * gpn_spconv_pack_weights writes the MFMA-fragment layout the kernels read:
 *   flags bit0 = transpose (use W_k^T: Cin/Cout swap), bit1 = reverse taps (k -> K-1-k); dgrad of
 *   a SubM conv uses both, dgrad of down/inverse convs uses transpose only.
 *   cin/cout here are the dims of the *packed* operator (after the optional transpose); both must be
 *   multiples of 16.  packed size = K*cin*cout floats.
 * gpn_spconv_fwd: out[dst] = sum_k in[nbr[k][dst]] @ W_k over the tap-major neighbour table of a rulebook
 *   (nbr [K, n_dst] i32, -1 = no neighbour; out is fully overwritten).  in [n_src, cin], out [n_dst, cout].
 * gpn_spconv_wgrad: dW[k] = sum_{pairs of k} in[src]^T (x) dout[dst]  -> dW [K, cin, cout] canonical.
 *   cout <= 128 (GPN_ERR_ARG above: callers split dout into <= 128-column pieces, as hip_ops.conv_wgrad does); any cin.
 * ================================================================================================ */
#define GPN_PACK_TRANSPOSE 1
#define GPN_PACK_REVERSE 2
#define GPN_LAYOUT_OKI 4 /* weights stored as the spconv-2.x parameter [Cout][K][Cin] instead of canonical [K][Cin][Cout] */
int gpn_spconv_pack_weights(const float* W, int K, int cin_w, int cout_w, int flags, float* packed,
                            gpn_stream_t stream);
size_t gpn_spconv_fwd_ws_bytes(int K, int64_t n_dst, int cin, int cout);
/* which kernel gpn_spconv_fwd* runs this shape on, under the current selection knobs (host arithmetic, no device needed).
 * n_plan < 0: n_dst is the exact row count; n_plan >= 0: n_dst bounds a device-counted row count and n_plan is the host's
 * estimate of it (0 = none).  Returns kind | sums << 8 | affine << 9: kind 0 = nothing to do (n_dst == 0), 1 = masked-tile,
 * 2 = masked tap-split, 3 = direct (or its tap-split form), 4 = lock-step, 5 = no kernel takes it (GPN_ERR_ARG from the conv:
 * a device-counted layer that fits none of 1 - 3, or K < 1 or a width below 16);
 * sums / affine: that kernel's epilogue can accumulate BatchNorm column sums / apply an inference pass's BatchNorm. */
int gpn_spconv_fwd_route(int K, int64_t n_dst, int64_t n_plan, int cin, int cout);
int gpn_spconv_fwd(const float* in, const float* packed_w, const int32_t* nbr, int K, int64_t n_dst, int cin,
                   int cout, float* out, void* ws, size_t ws_bytes, gpn_stream_t stream);
/* pack + conv in one call (packed copy lives in the head of ws); cin_w/cout_w are the STORED weight's dims */
/* the same conv over a rulebook that carries a TILE ORDER (gpn_rulebook_tile_order): nbr_p = the neighbour table in
 * that order, perm = the destination row of every tile position.  Results are identical (a row's taps are summed in
 * the same order); tiles whose rows share their neighbour mask simply skip more taps.  nbr_p / perm may both be NULL. */
int gpn_spconv_fwd_ordered(const float* in, const float* packed_w, const int32_t* nbr, const int32_t* nbr_p,
                           const int32_t* perm, int K, int64_t n_dst, int cin, int cout, float* out, void* ws,
                           size_t ws_bytes, gpn_stream_t stream);
/* kernel selection knob: layers of >= min_tiles 16-row tiles run on the masked-tile kernel (csrc/spconv_tiles.hip), smaller
 * ones on the direct / lock-step kernels; results are identical.  min_tiles < 0 queries.  Returns the previous value. */
int64_t gpn_spconv_tiles_min_tiles(int64_t min_tiles);
/* layers with few (16-row tile, 16-column tile) units run the direct kernel in a tap-split form (2 or 4 waves per unit,
 * partial sums added in LDS in wave order; csrc/spconv_fwd.hip): thresholds in units, negative = unchanged, 0 = never. */
int gpn_spconv_direct_split(int64_t split4_below_units, int64_t split2_below_units);
/* kernel selection knob (round 6): k = 27 / 8 layers below the masked-tile kernel's size run on the masked tap-split kernel
 * (csrc/spconv_msplit.hip: a workgroup per row tile, its waves own tap ranges, dead taps skipped); mode 0 hands them back to the
 * direct kernel, mode < 0 leaves the setting.  force_nt (1 - 4, a divisor of the layer's column tiles) / force_sp (4 or 9) fix the
 * column tiles per workgroup / the waves per row tile for every layer instead of the built-in table (0 = table, < 0 = unchanged):
 * measurement and test knob.  Returns the previous mode. */
int gpn_spconv_msplit(int mode, int force_nt, int force_sp);
size_t gpn_spconv_fwd_w_ws_bytes(int K, int64_t n_dst, int cin, int cout);
int gpn_spconv_fwd_w(const float* in, const float* W, int K, int cin_w, int cout_w, int pack_flags, const int32_t* nbr,
                     int64_t n_dst, float* out, void* ws, size_t ws_bytes, gpn_stream_t stream);
size_t gpn_spconv_wgrad_ws_bytes(int K, int cin, int cout, int64_t n_dst);
int gpn_spconv_wgrad(const float* in, const float* dout, const int32_t* pair_src,
                     const int32_t* pair_dst, const int32_t* tile_off, int K, int64_t n_dst, int cin,
                     int cout, int flags /* GPN_LAYOUT_OKI: write dW as [Cout][K][Cin] */, float* dW, void* ws,
                     size_t ws_bytes, gpn_stream_t stream);

/* BN — BatchNorm1d over a feature matrix [N, C] fused with the residual add and ReLU that follow it in every block of
 * the reference network (network/backbone.py:40-49 relu(bn(conv(x)) [+ shortcut]); norm_fn = BatchNorm1d(eps=1e-4,
 * momentum=0.1), network/model.py:86).  C % 4 == 0.  res may be NULL; relu = 0/1.
 * train: batch statistics (biased variance) -> mean / invstd [C] outputs (saved for backward); running_mean/var (may be
 *   NULL) are updated in place with `momentum` and the unbiased variance, as torch.nn.BatchNorm1d does.
 * eval: caller passes mean = running_mean and invstd = 1/sqrt(running_var + eps).
 * bwd: y = forward output (ReLU mask), dy = its gradient -> dx, dres (NULL if no residual), dweight, dbias. */
size_t gpn_bn_ws_bytes(int64_t N, int C);
int gpn_bn_fwd_train(const float* x, const float* res, const float* weight, const float* bias, int64_t N, int C,
                     float eps, float momentum, int relu, float* y, float* mean, float* invstd, float* running_mean,
                     float* running_var, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_bn_fwd_eval(const float* x, const float* res, const float* weight, const float* bias, const float* mean,
                    const float* invstd, int64_t N, int C, int relu, float* y, gpn_stream_t stream);
int gpn_bn_bwd(const float* x, const float* y, const float* dy, const float* weight, const float* mean,
               const float* invstd, int64_t N, int C, int relu, int training, float* dx, float* dres, float* dweight,
               float* dbias, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* G — row gather voxels->points and its deterministic transpose (model.py:153,359,394).
 * out[i] = idx[i] >= 0 ? table[idx[i]] : 0.   bwd: dtable[r] = sum_{i: idx[i]==r} dout[i] using the
 * CSR (order,starts) of points grouped by row (ascending point order inside a row). */
int gpn_gather_rows(const float* table, const int32_t* idx, int64_t n, int C, float* out,
                    gpn_stream_t stream);
int gpn_scatter_rows_csr(const float* dout, const int32_t* order, const int32_t* starts,
                         int64_t n_rows, int C, float* dtable, gpn_stream_t stream);

/* ================================================================================================
 * U — layer-program executor for the sparse residual U-Net (network/backbone.py:8-165: ResBlock.forward 40-49,
 * UBlock.forward 126-141, SparseUNet.forward 150-155).  The reference walks ~200 spconv / BatchNorm modules per
 * forward from Python; here the host side describes the same walk once as a flat op list and one call runs every
 * conv / BN / concat launch of the forward (or of the backward, in reverse, accumulating gradients), so the step is
 * not bound by per-layer interpreter overhead.  All arrays are host memory; every pointer inside them is device memory.
 *   slot     : an activation matrix [rows, channels] (data) and, for backward, its gradient buffer (grad)
 *   rulebook : neighbour table of the map and of its transpose (dgrad), plus the (tap,dst)-ordered pair lists (wgrad)
 *   conv     : weight in parameter layout [Cout][K][Cin] (GPN_LAYOUT_OKI) and where its gradient goes
 *   bn       : BatchNorm1d parameters / running stats / saved batch stats / gradients
 *   op       : CONV dst = conv(src0)        | BN dst = act(bn(src0) [+ src1])   | CONCAT dst = [src0 | src1]
 * forward: training == 1 uses batch statistics (saved into save_mean / save_invstd, running stats updated);
 *          training == 0 uses the running statistics (save_invstd receives 1/sqrt(var+eps));
 *          training == GPN_NET_INFERENCE (round 6): running statistics, and the caller promises that NO backward pass follows -
 *          every BatchNorm that directly follows a conv is then applied in that conv launch's epilogue (same arithmetic per
 *          element, bit-equal outputs; the conv's own output slot and save_invstd stay unwritten): a validation step of the
 *          full model has no BatchNorm launch left but the proposal networks' first one (network/backbone.py:40-49).
 * backward: slots[].grad of the final slot holds d(loss)/d(output); slots[].grad_state must be 0 everywhere except
 *          slots that already hold a gradient (1).  Gradients of multiply-consumed slots are summed in program order
 *          (reverse), so results are deterministic.  need_input_grad = 0 skips d/d(slot 0).
 * errors:  every pass validates ALL its tables, then its workspace size, before its first launch: GPN_ERR_ARG / GPN_ERR_WS leave
 *          nothing enqueued.  A BatchNorm over running statistics (training == 0 or GPN_NET_INFERENCE) needs weight, bias,
 *          running_mean and running_var, whether it is applied by a conv launch or by its own. */
typedef struct gpn_net_slot {
  float* data;
  float* grad;
  int64_t rows;
  int32_t channels;
  int32_t grad_state;
  /* Row counts that are still on the device (round 4: a pass issued without a host read of its sizes).  rows_dev != NULL:
   * `rows` is the BOUND the buffers (and the rulebook tables) are allocated for and *rows_dev the live row count, written by an
   * earlier launch on the same stream; every kernel of the pass reads it and walks its rows with a grid stride, so no result
   * depends on the host's knowledge.  rows_plan (> 0) is the host's ESTIMATE of that count (e.g. the previous step's): it only
   * sizes grids and picks kernel variants.  Tables of such a pass use the LIVE count as their leading dimension (nbr is
   * [K][*rows_dev], tile_off [K][ceil(*rows_dev / 32) + 1]) - exactly the layout of an exactly-sized pass, in larger buffers.
   * rows_dev == NULL: `rows` is the exact count (rows_plan ignored). */
  const int64_t* rows_dev;
  int64_t rows_plan;
} gpn_net_slot_t;
typedef struct gpn_net_rulebook {
  const int32_t* nbr;   /* [K][n_dst]  forward table */
  const int32_t* nbr_t; /* [K][n_src]  table of the transposed map */
  const int32_t* nbr_p;   /* optional tile order of the forward map (gpn_rulebook_tile_order): table ... */
  const int32_t* perm;    /* ... and destination rows; both NULL if absent */
  const int32_t* nbr_t_p; /* the same for the transposed map */
  const int32_t* perm_t;
  const int32_t* pair_src;
  const int32_t* pair_dst;
  const int32_t* tile_off;
  int64_t n_src;
  int64_t n_dst;
  int32_t K;
  int32_t reverse_taps; /* 1: SubM (transposed map = same table with taps reversed) */
} gpn_net_rulebook_t;
typedef struct gpn_net_conv {
  const float* W;
  float* dW;
  int32_t cin;
  int32_t cout;
} gpn_net_conv_t;
typedef struct gpn_net_bn {
  const float* weight;
  const float* bias;
  float* running_mean;
  float* running_var;
  float* save_mean;
  float* save_invstd;
  float* dweight;
  float* dbias;
  float eps;
  float momentum;
  int32_t C;
  int32_t reserved;
} gpn_net_bn_t;
#define GPN_NET_CONV 0
#define GPN_NET_BN 1
#define GPN_NET_CONCAT 2
#define GPN_NET_RELU 1 /* op.flags, BN only */
#define GPN_NET_INFERENCE 2 /* gpn_net_forward(_pair)'s `training`: eval mode without a backward pass to follow (see above) */
typedef struct gpn_net_op {
  int32_t kind;
  int32_t src0;
  int32_t src1; /* BN: residual slot or -1; CONCAT: right-hand input */
  int32_t dst;
  int32_t rulebook; /* CONV */
  int32_t param;    /* CONV: index into convs; BN: index into bns */
  int32_t flags;
  int32_t reserved;
} gpn_net_op_t;
/* training-mode BatchNorm sums (forward: sum x, sum x^2 of a conv's output; backward: sum g, sum g xhat of the gradient a dgrad
 * conv writes) are accumulated by the epilogue of the producing conv launch as order-independent 64-bit fixed-point integers
 * (csrc/bn_stats.h), so that a conv + BatchNorm pair costs 2 launches per direction instead of 3.  on = 0 restores the separate
 * statistics launches (results agree to ~1e-7 relative; both forms are deterministic).  on < 0 queries.  Returns the previous
 * setting. */
int gpn_net_bn_fusion(int on);
/* consecutive weight-gradient contractions of one shape (the convs of a level's residual blocks, the two networks of a paired
 * pass) that share a launch on the executor's second stream: 1 ... 4 layers (default 4, env GPN_WGRAD_GROUP; only layers with
 * fewer than GPN_WGRAD_GROUP_ROWS = 16384 rows are held back for it).  Same arithmetic per layer for every setting (bit-equal
 * gradients).  layers < 1 queries.  Returns the previous setting. */
int gpn_net_wgrad_group(int layers);
size_t gpn_net_ws_bytes(const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, int n_slots,
                        const gpn_net_rulebook_t* rulebooks, const gpn_net_conv_t* convs);
int gpn_net_forward(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots,
                    const gpn_net_rulebook_t* rulebooks, int n_rulebooks, const gpn_net_conv_t* convs, int n_convs,
                    const gpn_net_bn_t* bns, int n_bns, int training, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_net_backward(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots,
                     const gpn_net_rulebook_t* rulebooks, int n_rulebooks, const gpn_net_conv_t* convs, int n_convs,
                     const gpn_net_bn_t* bns, int n_bns, int training, int need_input_grad, void* ws, size_t ws_bytes,
                     gpn_stream_t stream);
/* Paired passes: TWO networks with the same program over the same rulebooks (the ScoreNet and NPCS-Net U-Nets of
 * network/model.py:116-118 read the same proposal grid), layer i of both computed by ONE launch per kernel (blockIdx.y picks
 * the network).  Each network's values are those of its own single pass.  Tables a / b: the two networks' slots, weights and
 * BatchNorms; ops and rulebooks are shared.  Workspace: 2 x gpn_net_ws_bytes. */
int gpn_net_forward_pair(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots_a, gpn_net_slot_t* slots_b, int n_slots,
                         const gpn_net_rulebook_t* rulebooks, int n_rulebooks, const gpn_net_conv_t* convs_a,
                         const gpn_net_conv_t* convs_b, int n_convs, const gpn_net_bn_t* bns_a, const gpn_net_bn_t* bns_b,
                         int n_bns, int training, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_net_backward_pair(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots_a, gpn_net_slot_t* slots_b, int n_slots,
                          const gpn_net_rulebook_t* rulebooks, int n_rulebooks, const gpn_net_conv_t* convs_a,
                          const gpn_net_conv_t* convs_b, int n_convs, const gpn_net_bn_t* bns_a, const gpn_net_bn_t* bns_b,
                          int n_bns, int training, int need_input_grad, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * C16 - opt-in reduced-precision INFERENCE path (csrc/spconv_bf16.hip): forward only, off by default, separate entry points;
 * nothing of the fp32 path runs through it.  bf16 tensors are passed as uint16_t (the upper half of the fp32 bit pattern).
 * Numerics contract: operands (activations, weights) are bf16; a product of two bf16 values is exact in fp32; sums are fp32
 * (v_mfma_f32_16x16x32_bf16, and v_mfma_f32_16x16x16_bf16 for the odd 16-channel block of the widths 16, 48, 80, 112), in a
 * fixed order - the 32-channel blocks of all taps one chain (ascending tap, within a tap ascending block), the odd 16-channel
 * block of all taps a second chain, result = chain32 + chain16 - that does not depend on the tile order or on the kernel
 * instantiation; taps a row does not have contribute exact zeros; launches are deterministic.  The epilogue runs in fp32 and a
 * stored activation is rounded ONCE, to nearest even; the network's output is fp32, unrounded.
 *   gpn_spconv_pack_weights_bf16: fp32 weight, canonical [K][Cin][Cout] (flags = 0) or parameter layout [Cout][K][Cin]
 *     (flags = GPN_LAYOUT_OKI; no other flag), -> K*cin*cout bf16 in the kernel's fragment order, each rounded to nearest even.
 *   gpn_spconv_fwd_bf16: in [n_src, cin] bf16, the tables of gpn_spconv_fwd_ordered (nbr [K][n_dst], -1 = none; nbr_p / perm the
 *     optional tile order, both or neither), 1 <= K <= 27, cin / 16 in {1..8, 10, 12, 14}, cout % 16 == 0,
 *     8 n_dst * 2 max(cin, cout) < 2^31 (32-bit byte offsets; GPN_ERR_ARG beyond).  Epilogue per output element, in fp32:
 *       v = (acc - mean) * (1 / sqrtf(var + eps)) * weight + bias     (mean != NULL; var, weight, bias then required)
 *       v += res[e]                                                   (res != NULL: bf16 [n_dst, cout], widened exactly)
 *       v = max(0, v)                                                 (relu)
 *     then out [n_dst, cout] = v rounded to bf16 (out_f32 == 0) or v itself as fp32 (out_f32 != 0).  ep == NULL: no epilogue,
 *     bf16 out.  Every output row is written once by one wave: no workspace.
 *   gpn_rows_to_bf16: y = x rounded to nearest even, [n, C].
 *   gpn_bn_act_bf16: y = act(bn_eval(x) [+ res]) with the epilogue's arithmetic on a tensor no conv produced; x fp32
 *     (x_is_f32 != 0) or bf16, y bf16.
 *   gpn_net_forward_bf16: the op program of section U over the same tables as gpn_net_forward in GPN_NET_INFERENCE mode (running
 *     statistics; a BatchNorm that directly and solely follows a conv is applied in that conv's epilogue).  slots[0].data is the
 *     fp32 input; the output slot (the one slot that is written and never read) receives fp32, unrounded; every other slot's
 *     data / grad is ignored and may be NULL: interior activations live in the workspace as bf16, one buffer per slot that is
 *     materialised.  A BatchNorm that reads slot 0 reads the fp32 input; every other reader of slot 0 reads its bf16 rounding.
 *     Weights are packed to bf16 into the workspace on every call.  Before the first launch the program is validated as by
 *     gpn_net_forward, and: no slot may carry rows_dev, conv widths must be supported by gpn_spconv_fwd_bf16, every BatchNorm
 *     needs weight, bias, running_mean and running_var, the workspace must hold gpn_net_forward_bf16_ws_bytes. */
typedef struct gpn_conv_epilogue_bf16 {
  const float* mean;
  const float* var;
  const float* weight;
  const float* bias;
  const uint16_t* res;
  float eps;
  int32_t relu;
  int32_t out_f32;
} gpn_conv_epilogue_bf16_t;
int gpn_spconv_pack_weights_bf16(const float* W, int K, int cin_w, int cout_w, int flags, uint16_t* packed, gpn_stream_t stream);
int gpn_spconv_fwd_bf16(const uint16_t* in, const uint16_t* packed_w, const int32_t* nbr, const int32_t* nbr_p, const int32_t* perm,
                        int K, int64_t n_dst, int cin, int cout, const gpn_conv_epilogue_bf16_t* ep, void* out, gpn_stream_t stream);
int gpn_rows_to_bf16(const float* x, int64_t n, int C, uint16_t* y, gpn_stream_t stream);
int gpn_bn_act_bf16(const void* x, int x_is_f32, const uint16_t* res, const float* weight, const float* bias, const float* mean,
                    const float* var, float eps, int64_t N, int C, int relu, uint16_t* y, gpn_stream_t stream);
size_t gpn_net_forward_bf16_ws_bytes(const gpn_net_op_t* ops, int n_ops, const gpn_net_slot_t* slots, int n_slots,
                                     const gpn_net_rulebook_t* rulebooks, const gpn_net_conv_t* convs);
int gpn_net_forward_bf16(const gpn_net_op_t* ops, int n_ops, gpn_net_slot_t* slots, int n_slots,
                         const gpn_net_rulebook_t* rulebooks, int n_rulebooks, const gpn_net_conv_t* convs, int n_convs,
                         const gpn_net_bn_t* bns, int n_bns, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * B — ball query.  replaces epic_ops.ball_query.ball_query (network/grouping_utils.py:119-128).
 * points [Np,3], query [Q,3], batch_indices [Q] i32, batch_offsets [S+1] i32 (CSR over points),
 * point_labels [Np] / query_labels [Q] i32 (both may be NULL = no label filter).
 * hit: same segment, equal label, d2 < radius^2 (strict; d2 = (dx*dx+dy*dy)+dz*dz, fp32, no fma),
 * first K hits in ascending point index.  indices [Q,K] i32 (-1 padded), count [Q] i32.
 * ================================================================================================ */
int gpn_ball_query(const float* points, const float* query, const int32_t* batch_indices,
                   const int32_t* batch_offsets, const int32_t* point_labels,
                   const int32_t* query_labels, int64_t Np, int64_t Q, int64_t S, float radius, int K,
                   int32_t* indices, int32_t* count, gpn_stream_t stream);
/* same contract and results, O(n k) instead of O(n^2): points binned into a uniform grid (one radix sort), one wave per
 * query over its 27 neighbour cells, hits ranked back into ascending point index; dense neighbourhoods fall back to the
 * index-order scan inside the kernel. */
/* Labels < 0 mark INACTIVE points / queries (grid form only): an inactive point is never a hit, an inactive query gets
 * count 0 - lets a caller run the query over a whole batch with the unwanted points masked instead of compacted away
 * (gpn_proposals_build).  K | GPN_BQ_NO_PAD: rows are not -1 filled beyond count[q] (saves a Q*K*4-byte fill). */
#define GPN_BQ_NO_PAD (1 << 30)
size_t gpn_ball_query_grid_ws_bytes(int64_t Np);
int gpn_ball_query_grid(const float* points, const float* query, const int32_t* batch_indices,
                        const int32_t* batch_offsets, const int32_t* point_labels, const int32_t* query_labels,
                        int64_t Np, int64_t Q, int64_t S, float radius, int K, int32_t* indices, int32_t* count, void* ws,
                        size_t ws_bytes, gpn_stream_t stream);

/* L — connected components.  replaces epic_ops.ccl.connected_components_labeling
 * (network/grouping_utils.py:135-137).  begin_end [2Q] i32 interleaved (begin,end) into edges [E];
 * edges are treated as undirected; labels [Q] i32 = minimum vertex index of the component.
 * compacted != 0 -> labels renumbered 0..n_comp-1 in order of that minimum (needs ws). */
size_t gpn_ccl_ws_bytes(int64_t Q);
int gpn_ccl(const int32_t* begin_end, const int32_t* edges, int64_t Q, int64_t E, int compacted,
            int32_t* labels, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* R — segmented reductions.  replace epic_ops.reduce.segmented_reduce (grouping_utils.py:59-70) and
 * epic_ops.reduce.segmented_maxpool (model.py:360-362).  values [M,C], begin/end [P] i32.
 * mode 0=sum 1=min 2=max; summation in ascending row order. empty segment -> 0.
 * maxpool: ties -> lowest row; argmax [P,C] i32 (-1 for empty). bwd scatters dpooled to drows. */
int gpn_segmented_reduce(const float* values, const int32_t* begin, const int32_t* end, int64_t P,
                         int C, int mode, float* out, gpn_stream_t stream);
int gpn_segmented_maxpool_fwd(const float* values, const int32_t* begin, const int32_t* end, int64_t P,
                              int C, float* pooled, int32_t* argmax, gpn_stream_t stream);
int gpn_segmented_maxpool_bwd(const float* dpooled, const int32_t* argmax, int64_t P, int C, int64_t M,
                              float* dvalues, gpn_stream_t stream);

/* I — instance IoU.  replaces epic_ops.iou.batch_instance_seg_iou (model.py:373-378).
 * proposal_offsets [P+1] i32, instance_labels [M] i32, batch_indices [M] i32,
 * num_points_per_instance [B,I] i32 -> ious [P,I] f32. */
int gpn_instance_iou(const int32_t* proposal_offsets, const int32_t* instance_labels,
                     const int32_t* batch_indices, const int32_t* num_points_per_instance, int64_t P,
                     int64_t B, int I, float* ious, gpn_stream_t stream);

/* N — greedy NMS on a precomputed IoU matrix.  replaces epic_ops.nms.nms (grouping_utils.py:244).
 * ious [P,P] f32, order [P] i32 = proposal ids by descending score (ties -> lower id; the host
 * wrapper sorts).  keep [P] i32 receives kept ids in visiting order, num_keep [1] i32. */
size_t gpn_nms_ws_bytes(int64_t P);
int gpn_nms(const float* ious, const int32_t* order, int64_t P, float threshold, int32_t* keep,
            int32_t* num_keep, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * F — PointNet++ family.  replace the pybind module pointnet2_cuda
 * (dataset/process_tools/utils/pointnet_lib/src/pointnet2_api.cpp:10-25); argument order and meaning
 * follow the vendored wrappers (ball_query.cpp:14-25, sampling.cpp, interpolate.cpp, group_points.cpp).
 * ================================================================================================ */
/* ball_query_gpu.cu:9-45 — first nsample (d2<r2) in index order; row prefilled with first hit;
 * rows without hits are left untouched. */
int gpn_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float* new_xyz,
                       const float* xyz, int32_t* idx, gpn_stream_t stream);
/* group_points_gpu.cu:47-66 / :8-25 */
int gpn_pn2_group_points(int b, int c, int n, int npoints, int nsample, const float* points,
                         const int32_t* idx, float* out, gpn_stream_t stream);
int gpn_pn2_group_points_grad(int b, int c, int n, int npoints, int nsample, const float* grad_out,
                              const int32_t* idx, float* grad_points, gpn_stream_t stream);
/* sampling_gpu.cu:8-24 / :46-63 */
int gpn_pn2_gather_points(int b, int c, int n, int npoints, const float* points, const int32_t* idx,
                          float* out, gpn_stream_t stream);
int gpn_pn2_gather_points_grad(int b, int c, int n, int npoints, const float* grad_out,
                               const int32_t* idx, float* grad_points, gpn_stream_t stream);
/* sampling_gpu.cu:93-209 — start index 0; temp [b,n] must be pre-filled with 1e10 by the caller
 * (pointnet2_utils.py:27); ties resolved as the reference's block reduction does for its block size
 * opt_n_threads(n) (cuda_utils.h:10-14). */
int gpn_pn2_furthest_point_sampling(int b, int n, int m, const float* dataset, float* temp,
                                    int32_t* idxs, gpn_stream_t stream);
/* same samples; clouds of >= 65536 points are shared by several workgroups (the pre-processing call,
 * dataset/process_tools/convert_rendered_into_input.py:115 of the reference: N ~ 1e5..1e6 -> 20 000). ws may be NULL when
 * gpn_pn2_furthest_point_sampling_ws_bytes returns 0. */
size_t gpn_pn2_furthest_point_sampling_ws_bytes(int b, int n);
int gpn_pn2_furthest_point_sampling_ws(int b, int n, int m, const float* dataset, float* temp, int32_t* idxs,
                                       void* ws, size_t ws_bytes, gpn_stream_t stream);
/* interpolate_gpu.cu:81-124 / :9-57 / :149-169 / :192-214 */
int gpn_pn2_three_nn(int b, int n, int m, const float* unknown, const float* known, float* dist2,
                     int32_t* idx, gpn_stream_t stream);
int gpn_pn2_knn(int b, int n, int m, int k, const float* unknown, const float* known, float* dist2,
                int32_t* idx, gpn_stream_t stream);
int gpn_pn2_three_interpolate(int b, int c, int m, int n, const float* points, const int32_t* idx,
                              const float* weight, float* out, gpn_stream_t stream);
int gpn_pn2_three_interpolate_grad(int b, int c, int n, int m, const float* grad_out,
                                   const int32_t* idx, const float* weight, float* grad_points,
                                   gpn_stream_t stream);

/* ================================================================================================
 * P — per-point losses of the training step in one pass (network/model.py:177-226: loss_sem_seg = focal (gamma 2, rows with
 * label == ignore_index dropped, 0 if none is left) + dice on the 1e-6-smoothed one-hot target; loss_offset = L1 distance
 * and negative cosine on points with label > 0 and instance label >= 0; network/losses.py:35-64, 111-158).
 * logits [M,C] (C <= 32), labels [M] i64, offsets / gt_offsets [M,3], instance_labels [M] i32.
 * fwd -> losses [4] f32 = (focal, dice, offset distance, offset direction) and a 32-byte device block `stats` for bwd;
 * bwd: grad_losses [4] f32 (device) -> d_logits [M,C], d_offsets [M,3].  Fixed-order reductions (deterministic).
 * ================================================================================================ */
size_t gpn_point_losses_ws_bytes(int64_t M);
int gpn_point_losses_fwd(const float* logits, const int64_t* labels, const float* offsets, const float* gt_offsets,
                         const int32_t* instance_labels, int64_t M, int C, int64_t ignore_index, float* losses,
                         void* stats, void* ws, size_t ws_bytes, gpn_stream_t stream);
/* the same with the step's by-products of the logits: preds [M] i64 = the predicted class of every point (first maximum, as
 * torch.argmax), accu [2] f32 = (share of points with preds == labels, the same share among the points with labels > 0; both
 * as fp32 quotients of the exact counts - network/model.py:535-541) */
int gpn_point_losses_fwd_metrics(const float* logits, const int64_t* labels, const float* offsets, const float* gt_offsets,
                                 const int32_t* instance_labels, int64_t M, int C, int64_t ignore_index, float* losses,
                                 int64_t* preds, float* accu, void* stats_out, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_point_losses_bwd(const float* logits, const int64_t* labels, const float* offsets, const float* gt_offsets,
                         const int32_t* instance_labels, int64_t M, int C, int64_t ignore_index, const void* stats,
                         const float* grad_losses, float* d_logits, float* d_offsets, gpn_stream_t stream);

/* Proposal score loss in one launch: class selection (model.py:560-566 of the reference), get_gt_scores
 * (grouping_utils.py:144-156) on the row maxima of ious, binary_cross_entropy_with_logits (mean), plus sigmoid scores and
 * d loss / d logits.  logits [P, C1]; cls_i64 / cls_i32 [M]: class of every proposal point (exactly one non-NULL); offsets
 * [P+1] i32; ious [P, I] (gpn_instance_iou).  Outputs: loss [1], score_preds [P], d_logits [P, C1]. */
int gpn_score_loss(const float* logits, int C1, const int64_t* cls_i64, const int32_t* cls_i32, const int32_t* offsets,
                   const float* ious, int I, int64_t P, float fg_thresh, float bg_thresh, float* loss, float* score_preds,
                   float* d_logits, gpn_stream_t stream);

/* NPCS loss of all proposals in two launches (+ one backward): network/model.py:398-462 with compute_npcs_loss
 * (network/grouping_utils.py:14-43).  logits [M, n_cls3 = 3 (classes - 1)], gt_npcs [M,3], sem_preds [M] i32 (one class per
 * proposal point), sem_labels [M] i64, proposal_offsets [P+1] i32 / proposal_indices [M] i64 (CSR of the proposals),
 * sym_of_class [classes] i64 (device), mats [n_mats,3,3] f32 (device): candidate rotations of every symmetry type back to
 * back; type_first / type_count (<= 24) / type_group (0..2) [n_types <= 8] on the HOST.  loss [1] f32 (device);
 * scratch: (9 P + 4) * 4 bytes kept by the caller between forward and backward.  d_logits [M, n_cls3] fully written. */
int gpn_npcs_loss_fwd(const float* logits, int n_cls3, const float* gt_npcs, const int32_t* sem_preds,
                      const int64_t* sem_labels, const int32_t* proposal_offsets, int64_t P, const int64_t* sym_of_class,
                      const float* mats, const int32_t* type_first, const int32_t* type_count, const int32_t* type_group,
                      int n_types, float* loss, void* scratch, gpn_stream_t stream);
int gpn_npcs_loss_bwd(const float* logits, int n_cls3, const float* gt_npcs, const int32_t* sem_preds,
                      const int64_t* sem_labels, const int64_t* proposal_indices, int64_t M, int64_t P,
                      const int64_t* sym_of_class, const float* mats, const int32_t* type_first, const int32_t* type_count,
                      const int32_t* type_group, int n_types, const void* scratch, const float* grad_loss, float* d_logits,
                      gpn_stream_t stream);

/* ================================================================================================
 * PR — the proposal stage of a step in one call: GAPartNet.proposal_clustering_and_revoxelize (network/model.py:228-346)
 * with cluster_proposals (network/grouping_utils.py:108-140) and the geometry of segmented_voxelize (:47-104).
 * Inputs: points [N, point_stride] f32 (xyz = first three columns), offset_preds [N,3] f32, sem_preds [N] i64 (arg-max of
 * the semantic head), instance_labels [N] i32 or NULL, batch_indices [N] i32 (scene of every point, non-decreasing),
 * jitter [6] f32 on the DEVICE = the two uniform 3-vectors of grouping_utils.py:86-90.
 * A point is valid if sem_preds > 0 (and instance_labels >= 0 when given).  Both cluster sets (xyz, xyz + offset; radius,
 * K1 / K2 neighbours, label-aware) -> proposals of >= min_points points, ordered by their first point, members ascending,
 * set A's proposals before set B's -> per-proposal frame (centre, scale <= max_scale, jittered shift) -> fullscale^3 voxel
 * grid per proposal.  Nothing is read back: every output has its upper-bound capacity and counts [8] i64 (device) holds
 * {Q valid points, M proposal points, P proposals, V voxels, points dropped by the voxeliser, (internal), rows of the grid's
 * stride-2 level, (unused)}.  The stride-2 rows are counted as gpn_rulebook_level_counts counts them: distinct
 * (proposal, x/2, y/2, z/2) rows inside the coarse grid of floor(fullscale/2)^3 cells, so with an odd fullscale the voxels
 * at x == fullscale - 1 (any axis) do not count.
 * Outputs (capacity): valid_mask [N] u8, valid_indices [N] i64; per proposal point [2N]: sorted_indices i64 (numbering
 * among the valid points, as the reference), point_indices i64 (row of `points`), proposal_indices i64, batch_indices_p
 * i32, pt_xyz_p [.,3] f32, sem_preds_p i32, instance_labels_p i32, pc_voxel_id i32, point_order i32 (+ voxel_point_start
 * [2N+1] i32: points grouped by voxel); member_slot [2N] i32 (row of the proposal-point list holding point i in set A
 * (entry i) / set B (entry N+i), -1 if none); per proposal [gpn_proposals_max_proposals + 1]: sizes i64,
 * proposal_offsets i32; voxel_coords4 [2N,4] i32 = (proposal, x, y, z), ordered.
 * gpn_proposals_voxel_mean(_bwd): voxel features = ordered mean of feats[point_indices] over each voxel's points, and its
 * transpose (each point sums its at most two memberships in fixed order) - the differentiable half of kernel V.
 * ================================================================================================ */
int64_t gpn_proposals_max_proposals(int64_t N, int min_points);
size_t gpn_proposals_build_ws_bytes(int64_t N, int64_t B, int K1, int K2, int min_points);
int gpn_proposals_build(const float* points, int point_stride, const float* offset_preds, const int64_t* sem_preds,
                        const int32_t* instance_labels, const int32_t* batch_indices, int64_t N, int64_t B, float radius,
                        int K1, int K2, int min_points, float fullscale, float max_scale, const float* jitter,
                        int64_t* counts, uint8_t* valid_mask, int64_t* valid_indices, int64_t* sorted_indices,
                        int64_t* point_indices, int64_t* proposal_indices, int32_t* batch_indices_p, float* pt_xyz_p,
                        int32_t* sem_preds_p, int32_t* instance_labels_p, int64_t* sizes, int32_t* proposal_offsets,
                        int32_t* member_slot, int32_t* voxel_coords4, int32_t* pc_voxel_id, int32_t* point_order,
                        int32_t* voxel_point_start, void* ws, size_t ws_bytes, gpn_stream_t stream);
/* the re-voxelisation step of gpn_proposals_build on its own: the points of the proposals (grouped by proposal, ascending
 * point order inside one; scaled [T2,3] = coordinates in the proposal's grid of (fullscale + 1)^3 unit cells, kept when
 * 0 <= c < fullscale on every axis) -> what gpn_voxelize_ex gives for them with the proposals as segments - unique cells in
 * (proposal, x, y, z) order, voxel of every point (-1 = outside its grid), points grouped by voxel in ascending point order
 * (point_order [T2], voxel_point_start [V + 1]; the dropped points behind all others) - WITHOUT a sort: one workgroup per
 * proposal keeps the grid's bitmap and per-cell counts in LDS.  counts = the stage's count block on the device: [1] = points
 * and [2] = proposals are read, [3] = voxels is written.  fullscale <= 30. */
size_t gpn_proposals_revoxelize_ws_bytes(int64_t P_ub);
int gpn_proposals_revoxelize(const float* scaled, const int32_t* proposal_offsets, int64_t* counts, int64_t T2, int64_t P_ub,
                             float fullscale, int32_t* voxel_coords3, int32_t* voxel_seg, int32_t* pc_voxel_id,
                             int32_t* point_order, int32_t* voxel_point_start, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_proposals_voxel_mean(const float* feats, const int64_t* point_indices, const int32_t* point_order,
                             const int32_t* voxel_point_start, int64_t V, int C, float* out, gpn_stream_t stream);
int gpn_proposals_voxel_mean_bwd(const float* dout, const int32_t* member_slot, const int32_t* pc_voxel_id,
                                 const int32_t* voxel_point_start, int64_t N, int C, float* dfeats, gpn_stream_t stream);

/* ================================================================================================
 * MP - proposals from caller-supplied masks: the front of the proposal stage when the parts are GIVEN (point masks with a part
 * class each: a 2-D segmenter's masks lifted to the points) instead of found by clustering.  Serves the reference's deployment
 * calls estimate_pose_from_mask / forward_with_masks (structure/utils.py:195-322); the contract is chosen from those call sites
 * (INTEGRATION.md).  Inference only: no member_slot, no backward, no gpn_proposals_postprocess behind it.
 * gpn_mask_pack: masks on the caller's rows -> bit sets on the network's points.  masks u8 (non-zero = member), mask k is the run
 * of bytes starting at mask_base[k] (i64) over the rows of the caller's cloud mask_scene[k] (i32, non-decreasing; a scene may own
 * no mask); scene_offsets [S+1] i64 = the scenes' rows in the network batch; sample_rows [n_net] i64 = row of every network point
 * inside its caller's cloud, or NULL = identity.  bits [K, W] u64, W = ceil(max m_s / 64): bit (j & 63) of word (j >> 6) of mask
 * k is set iff network point scene_offsets[s] + j is a member; bits at and beyond m_s are zero.  One wave per word (ballot); only
 * the K m sampled bytes are read.
 * gpn_proposals_from_masks: the bit sets -> the tables of section PR.  A mask is kept iff it has >= min_points members and
 * 1 <= mask_label[k] < n_classes.  Proposals = the kept masks in the caller's order, members ascending; a point may sit in any
 * number of them.  valid_mask [N] u8 = member of at least one kept mask, valid_indices the valid points, sorted_indices the
 * numbering among them (row = valid_indices[sorted_indices]).  Per proposal point [M_cap]: sorted_indices, point_indices,
 * proposal_indices i64, batch_indices_p i32, pt_xyz_p [.,3] f32, sem_preds_p i32 = the mask's label, pc_voxel_id, point_order i32
 * (+ voxel_point_start [M_cap+1]); per proposal [K+1]: sizes i64, proposal_offsets i32, proposal_mask i64 = k; voxel_coords4
 * [M_cap,4].  Then the tail of gpn_proposals_build (frame, re-voxelisation into fullscale^3 grids - sort-free for fullscale <= 30,
 * the sorting voxeliser above - coarse-level rows).  counts [8] i64 (device): {Q, M, P, V, dropped, masks with a label outside
 * [1, n_classes), coarse rows, overflow}.  A member total above M_cap sets counts[7] to that total, leaves M = P = 0 and writes
 * no per-point row.  K = 0 (or no scene, W = 0, M_cap = 0): every count 0, valid_mask cleared.  Nothing is read back.
 * ================================================================================================ */
int gpn_mask_pack(const uint8_t* masks, const int64_t* mask_base, const int32_t* mask_scene, const int64_t* scene_offsets,
                  const int64_t* sample_rows, int64_t K, int64_t W, uint64_t* bits, gpn_stream_t stream);
size_t gpn_proposals_from_masks_ws_bytes(int64_t K, int64_t S, int64_t W, int64_t M_cap);
int gpn_proposals_from_masks(const uint64_t* bits, int64_t W, const int32_t* mask_scene, const int64_t* mask_label,
                             const int64_t* scene_offsets, const float* points, int point_stride, int64_t K, int64_t S, int64_t N,
                             int min_points, int n_classes, float fullscale, float max_scale, const float* jitter, int64_t M_cap,
                             int64_t* counts, uint8_t* valid_mask, int64_t* valid_indices, int64_t* sorted_indices,
                             int64_t* point_indices, int64_t* proposal_indices, int32_t* batch_indices_p, float* pt_xyz_p,
                             int32_t* sem_preds_p, int64_t* sizes, int32_t* proposal_offsets, int64_t* proposal_mask,
                             int32_t* voxel_coords4, int32_t* pc_voxel_id, int32_t* point_order, int32_t* voxel_point_start, void* ws,
                             size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * BP - the preparation of one batch for a sparse U-Net in ONE call (round 5): gpn_voxelize_scenes, its one host read, and the
 * rulebook pyramid of the backbone - per level the SubM k = 3 tables (+ tile order from tile_order_min_rows rows), the stride-2
 * map to the next level and its transpose (+ tile order), and, for the levels in the bit mask ident_levels, the k = 1 identity
 * map.  Replaces the loader's per-scene CPU voxelisation (dataset/gapartnet.py:179-205) and spconv's indice-pair construction
 * inside the forward pass (network/backbone.py:19-36, 74-90, 149-152) - the same launches as the separate entry points of
 * sections V / K1 / K2, issued from one native loop into ONE caller-allocated arena.  The call BLOCKS (a blocking-sync event on
 * `stream`) for the voxeliser's sizes; it may be called from any thread (`device` = HIP device ordinal, set for the calling
 * thread) - measured, a worker thread loses to calling it inline (csrc/prepare.hip).
 * desc_host [gpn_backbone_prepare_desc_words(n_levels)] i64, HOST memory; offsets are bytes from the arena base, -1 = absent:
 *   [0] voxels V  [1..3] spatial shape of level 0  [4] dropped points  [5] != 0: fall back to the separate calls (a cell index
 *   beyond the packed keys, an empty batch, an empty level)  [6] n_levels  [7] arena bytes used
 *   [8] voxel_feats [M,C] f32  [9] indices4 [M,4] i32  [10] pc_voxel_id [M] i32  [11] point_order [M] i32  [12] voxel_point_start [M+1]
 *   level l at 16 + 48 l: rows, shape[3], indices offset ([rows,4] i32), 3 spare, then 4 rulebooks x 10 words
 *   (SubM, down = dst coarse, its transpose = dst fine, identity): nbr, pair_src, pair_dst, tile_off, num_pairs, nbr_p, perm
 *   (offsets), n_src, n_dst, K.  Pair lists have the capacities of the separate entry points (27 n, n fine rows, n).
 * pinned_stats_host [8 + n_levels] i64: pinned host memory the statistics are copied to.
 * ================================================================================================ */
int gpn_backbone_prepare_desc_words(int n_levels);
size_t gpn_backbone_prepare_arena_bytes(int64_t M, int C, int64_t S, int n_levels);
int gpn_backbone_prepare(const float* points, const float* feats, const int64_t* seg_offsets, int64_t M, int C, int64_t S,
                         const float* voxel_size_host, int n_levels, uint32_t ident_levels, int64_t tile_order_min_rows,
                         int tile_order_block, int device, void* arena, size_t arena_bytes, int64_t* desc_host,
                         int64_t* pinned_stats_host, gpn_stream_t stream);

/* ================================================================================================
 * SP - the per-scene preparation of RAW scenes for a whole batch (round 5): what the reference's loader workers do per scene in
 * numpy (dataset/gapartnet.py:55-82) - compact_instance_labels (:134-142), apply_augmentations (:85-120; the random draws stay
 * on the host, 9 + C doubles per scene come in), generate_inst_info (:145-176) - in three launches.
 * Inputs: points [N, 3 + C] f32 (scenes back to back, seg_offsets [B + 1] i64 on the device), sem_labels [N] (sem_bytes = 2 / 4 / 8:
 * int16 / int32 / int64), instance_labels [N] i32 (negative = no instance), mats [B, 3, 3] f64 or NULL (xyz @ M in float64, rounded
 * once), shifts [B, C] f64 or NULL (colour + shift in float64, rounded once).
 * Outputs: points_out [N, 3 + C]; batch_indices [N] i32; instance_out [N] i32 (the non-negative ids of every scene renumbered
 * 0..K-1 ascending; negatives kept); regions [N, 9] f32 = mean | min | max xyz of the point's instance (zeros off-instance; the mean
 * from an order-independent fixed-point sum, within an ulp of numpy's); num_points_per_instance / instance_sem_labels
 * [B, gpn_scene_prepare_max_instances()] i32 (count, semantic label of the instance's first point; 0 / -1 past a scene's K);
 * num_instances_host [B] i64 = K per scene, written by the device into PINNED host memory (or NULL), -1 for a scene with more
 * distinct ids than the tables hold - *overflow (device) is then 1 and the outputs are not to be used. */
int gpn_scene_prepare_max_instances(void);
size_t gpn_scene_prepare_ws_bytes(int B);
int gpn_scene_prepare(const float* points, const void* sem_labels, int sem_bytes, const int32_t* instance_labels,
                      const int64_t* seg_offsets, int64_t N, int C, int B, const double* mats, const double* shifts,
                      float* points_out, int32_t* batch_indices, int32_t* instance_out, float* regions,
                      int32_t* num_points_per_instance, int32_t* instance_sem_labels, int64_t* num_instances_host,
                      int32_t* overflow, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * PP - post-processing of a validation / test step's proposals in one call (round 5): filter_invalid_proposals +
 * apply_nms of the reference (network/grouping_utils.py:159-298, called from network/model.py:667-692, 807-857).
 * Inputs as gpn_proposals_build left them: score_preds [P] f32 (the sigmoid scores), sizes [P] i64, proposal_offsets [P+1] i32,
 * point_indices / proposal_indices [M] i64, member_slot [2N] i32 (N = points of the batch).  P may be a bound with the live count
 * in *p_dev (p_plan sizes grids only).  A proposal survives if score > score_threshold and size > min_points (both strict) and
 * greedy NMS by descending score (ties: lower id first) on the point-set IoU inter / ((|a| + |b|) - inter + 1e-8) (fp32) does
 * not suppress it (IoU > iou_threshold with a kept proposal of higher rank).
 * Outputs: kept_ids [P] i32 = ids of the kept proposals, ascending; new_offsets [P+1] i32 = their CSR offsets after compaction;
 * src_row [M] i64 = for every point of a kept proposal its row in the inputs; counts [3] i64 (device) = {kept proposals, their
 * points, != 0: a proposal shared points with more proposals than the kernel tables hold (results incomplete)}.  The caller
 * re-indexes whatever per-proposal / per-point fields it needs with kept_ids / src_row. */
size_t gpn_proposals_postprocess_ws_bytes(int64_t P);
int gpn_proposals_postprocess(const float* score_preds, const int64_t* sizes, const int32_t* proposal_offsets,
                              const int64_t* point_indices, const int64_t* proposal_indices, const int32_t* member_slot, int64_t N,
                              int64_t P, const int64_t* p_dev, int64_t p_plan, float score_threshold, int64_t min_points,
                              float iou_threshold, int32_t* kept_ids, int32_t* new_offsets, int64_t* src_row, int64_t* counts,
                              void* ws, size_t ws_bytes, gpn_stream_t stream);
/* The NMS kernel keeps one status byte per LIVE proposal in LDS up to n proposals (default and maximum 131072) and in the
 * workspace beyond - any bound P is accepted (round 5 rejected bounds above 131072: 32 scenes of 20k points).  n < 0 queries;
 * returns the previous value.  Tests lower it to run the workspace form on small inputs. */
int64_t gpn_proposals_postprocess_lds_proposals(int64_t n);

/* ================================================================================================
 * O — the optimizer step.  GAPartNet.configure_optimizers (network/model.py:1051-1055): torch.optim.Adam(lr) over every
 * parameter.  One launch for the whole model: table [n_tensors] on the DEVICE describes the fp32 tensors (built once;
 * pointers are stable from step to step), block_first [n_tensors] i32 = first workgroup of each tensor with
 * gpn_adam_blocks(numel) workgroups per tensor.  Update = torch's single-tensor Adam in fp32 (no amsgrad, no weight decay),
 * `step` = the 1-based step count shared by the tensors of the call.
 * ================================================================================================ */
typedef struct {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  int64_t numel;
} gpn_adam_tensor_t;
/* n_segs fp32 segments dst[0..numel) = src[0..numel) (device memory) in one launch per 96 segments; segs_host is read during
 * the call.  (Gradients that autograd allocates afresh every step -> the persistent buffers an Adam table points at.) */
typedef struct {
  const void* src;
  void* dst;
  int64_t numel;
} gpn_copy_seg_t;
int gpn_copy_many(const gpn_copy_seg_t* segs_host, int n_segs, gpn_stream_t stream);
int gpn_adam_blocks(int64_t numel);
int gpn_adam_step(const gpn_adam_tensor_t* table_dev, const int32_t* block_first_dev, int n_tensors, int n_blocks, double lr,
                  double beta1, double beta2, double eps, int64_t step, gpn_stream_t stream);
/* the same step for tensors whose gradients exist only if a DEVICE counter is non-zero (round 5): the ScoreNet / NPCS-Net
 * parameters of a training step whose proposal count was never read on the host (section DEV).  The reference does not run
 * those networks for a batch without proposals (network/model.py:573-574: the gradients stay None and torch.optim.Adam skips
 * the tensors - value, moments and step count unchanged); the device-counted step runs them over zero rows and gets zero
 * gradients, which an ungated Adam step would still turn into a parameter update (momentum) and a moment decay.
 * *gate_dev == 0: nothing is touched and *skipped_dev += 1.  Otherwise the step number is step - *skipped_dev (>= 1).
 * gate_dev == skipped_dev == NULL: gpn_adam_step. */
int gpn_adam_step_gated(const gpn_adam_tensor_t* table_dev, const int32_t* block_first_dev, int n_tensors, int n_blocks,
                        double lr, double beta1, double beta2, double eps, int64_t step, const int64_t* gate_dev,
                        int64_t* skipped_dev, gpn_stream_t stream);

/* ================================================================================================
 * VP - rendered RGB-D views -> training scenes (the reference's dataset/process_tools/convert_rendered_into_input.py,
 * sample_and_save :90-175) for a batch of V views of one size H x W, in three launches with no host read between them.
 * Inputs per view: depth [H,W] f32 (depth_bytes 4) or f64 (8), sem / ins [H,W] i32 (-2 background, -1 "others"), rgb [H,W,3] u8,
 * npcs [H,W,3] f32, K [3,3] f64 row-major (meta['camera_intrinsic'] reshaped, :44).
 * gpn_view_backproject: valid pixels (sem != -2 and ins != -2, :55) in row-major order -> pixel [V, H*W] i32 (linear index),
 *   points [V, H*W, 4] f32 = the float32 cast of the float64 ((pix - c) * z) / f back-projection (:57-59) in .xyz, .w scratch;
 *   counts [V] i32 and status [V] i32 (GPN_VIEW_OK or GPN_VIEW_LABEL_MISMATCH, where the reference asserts, :112) on the device.
 * gpn_view_fps: per view with status OK, idx [V, m] i32 = gpn_pn2_furthest_point_sampling of that view's counts[v] points alone
 *   (utils/sample_utils.py:46-66: start 0, ties as the reference's block reduction for opt_n_threads(n)); counts[v] == m: arange;
 *   counts[v] < m: status GPN_VIEW_TOO_FEW (:116-117).  points [V, n_bound, 4] as above (.w is overwritten).  All views in one
 *   launch; several workgroups share a view and meet at a counter only under a cooperative launch whose grid is at most one
 *   workgroup per CU, otherwise one workgroup per view without any wait.  max_groups > 0 caps the workgroups per view (1: the
 *   wait-free form).
 * gpn_view_finish: per view with status OK, from the original maps: xyz [V,m,3] f32 = ball-normalised float64 points (:71-87,
 *   center (max + min) / 2, r = sqrt(max((dx^2 + dy^2) + dz^2))), rgb [V,m,3] f32 = u8 / 255.0, sem [V,m] = sem + 1, ins [V,m] =
 *   -1 -> -100 then the relabel loop (:142-147), npcs [V,m,3], pix [V,m,2] = (y, x), gt [V,m] = sem of the instance's first point
 *   * 1000 + id, -100 elsewhere (:162-171), scale [V,4] f64 = (r, cx, cy, cz).  A sampled instance id >=
 *   gpn_view_max_instance_ids() sets status GPN_VIEW_INSTANCE_BOUND (that view's outputs are not to be used).
 * ================================================================================================ */
#define GPN_VIEW_OK 0
#define GPN_VIEW_TOO_FEW 1
#define GPN_VIEW_LABEL_MISMATCH 2
#define GPN_VIEW_INSTANCE_BOUND 3
int gpn_view_max_instance_ids(void);
int gpn_view_backproject(const void* depth, int depth_bytes, const int32_t* sem, const int32_t* ins, const double* K, int V, int H,
                         int W, int32_t* pixel, float* points, int32_t* counts, int32_t* status, gpn_stream_t stream);
size_t gpn_view_fps_ws_bytes(int V);
int gpn_view_fps(float* points, int64_t n_bound, const int32_t* counts, int32_t* status, int V, int m, int max_groups, int32_t* idx,
                 void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_view_finish(const void* depth, int depth_bytes, const uint8_t* rgb, const int32_t* sem, const int32_t* ins, const float* npcs,
                    const double* K, int V, int H, int W, const int32_t* pixel, const int32_t* idx, int m, int32_t* status,
                    float* xyz, float* rgb_out, int32_t* sem_out, int32_t* ins_out, float* npcs_out, int32_t* pix_out, int32_t* gt,
                    double* scale, gpn_stream_t stream);

/* ================================================================================================
 * CP - label-free inference on raw point clouds: S ragged clouds -> the network's input, and per-sample predictions -> every row.
 * What the reference does on the CPU around `perception_model(pcs)` (tools/visu_utils.py:157-173 FindMaxDis / WorldSpaceToBallSpace,
 * structure/utils.py:345,613 FPS), plus what it has no answer for: the points that were not sampled.
 * points [M, stride] f32 with xyz in columns 0..2 (stride >= 3 = the row pitch in floats: a column slice of a wider array passes
 * the wide array's; gpn_cloud_finish takes the slice's own column count as `cols` <= stride),
 * offsets [S+1] i64 on the device: cloud s = rows offsets[s]:offsets[s+1].  A row is VALID when its three coordinates are finite.
 * gpn_cloud_pack: per cloud the valid rows in ascending row order (a scan, no atomic counter) -> packed [S, n_bound, 4] f32 = .xyz
 *   and .w = 1e10 (exactly what gpn_view_backproject writes: the layout gpn_view_fps reads), rows [S, n_bound] i32 = the row inside
 *   the caller's cloud, counts [S] i32, status [S] i32 = GPN_CLOUD_OK, or GPN_CLOUD_EMPTY when no row is valid.  n_bound >= the
 *   largest cloud's row count (rows past it are ignored).
 * Sampling is gpn_view_fps(packed, n_bound, counts, status, S, m, ...) as it is: GPN_CLOUD_OK == GPN_VIEW_OK, a cloud with
 *   counts[s] > m is sampled, == m gives arange, and < m is flagged GPN_CLOUD_FEW (== GPN_VIEW_TOO_FEW) with no indices written,
 *   which gpn_cloud_finish reads as "keep every valid point".
 * gpn_cloud_finish: per cloud over its m_s = min(counts[s], m) samples, in float64 from the caller's float32 rows: c = (max + min)
 *   / 2, r = sqrt(max((dx*dx + dy*dy) + dz*dz)), xyz = float32((p - c) / r) - the formula of gpn_view_finish.  DECISION: centre and
 *   radius are taken over the SAMPLED points, not the whole cloud - that is what the converter (section VP) does and so what the
 *   network was trained on.  out [S, m, cols] f32 = normalised xyz, the other columns copied bit for bit (rows past m_s zero),
 *   sample_rows [S, m] i32 = the caller's row (inside its cloud) of every sample (-1 past m_s), scale [S, 4] f64 = (r, cx, cy, cz).
 *   status: GPN_CLOUD_FEW becomes GPN_CLOUD_OK; r == 0 (one point, or all equal) sets GPN_CLOUD_DEGENERATE (xyz written as 0).
 * gpn_cloud_nearest: for every one of the M rows (sampled or not) the nearest sample of its own cloud, in the caller's coordinates:
 *   d2 = (dx*dx + dy*dy) + dz*dz in fp32 without fma (the convention of gpn_ball_query), ties to the lowest sample.  nn [M] i32 = the
 *   sample's position 0 .. m_s - 1 in its cloud; -1 for an invalid row, for every row of a cloud whose status is not GPN_CLOUD_OK
 *   and for rows outside [offsets[0], offsets[S]).  d2_out [M] f32 (may be NULL): that distance, +inf where nn is -1.  EXACT: a
 *   per-cloud uniform grid over the samples' box (at most 64 cells an axis; histogram, scan, stable scatter), each query walks
 *   Chebyshev rings of cells around its own (clamped) cell and stops when no unvisited ring can hold an equal or nearer sample;
 *   after 3 rings it scans all samples of the cloud (queries far outside the box, all samples in one cell).
 * ================================================================================================ */
#define GPN_CLOUD_OK 0
#define GPN_CLOUD_FEW 1
#define GPN_CLOUD_EMPTY 2
#define GPN_CLOUD_DEGENERATE 3
int gpn_cloud_pack(const float* points, int64_t M, int stride, const int64_t* offsets, int S, int64_t n_bound, float* packed,
                   int32_t* rows, int32_t* counts, int32_t* status, gpn_stream_t stream);
int gpn_cloud_finish(const float* points, int64_t M, int stride, int cols, const int64_t* offsets, int S, int64_t n_bound,
                     const int32_t* rows, const int32_t* counts, const int32_t* idx, int m, int32_t* status, float* out,
                     int32_t* sample_rows, double* scale, gpn_stream_t stream);
size_t gpn_cloud_nearest_ws_bytes(int S, int m);
int gpn_cloud_nearest(const float* points, int64_t M, int stride, const int64_t* offsets, int S, const int32_t* sample_rows,
                      const int32_t* counts, const int32_t* status, int m, int32_t* nn, float* d2_out, void* ws, size_t ws_bytes,
                      gpn_stream_t stream);

/* ================================================================================================
 * FR - RGB-D frames -> the rows and the packed layout of section CP: the front of the reference's deployment path
 * (structure/gapartnet.py:541-627 ObjIns.get_pc / get_downsampled_pc, structure/utils.py:454-476 get_point_cloud) for a batch of V
 * frames of one size H x W (V <= 65535).  No host read between the launches; no float atomics; integer atomics only on histograms
 * and counters, whose results do not depend on their order; every output is bit-reproducible.
 * gpn_frame_backproject: depth [V,H,W] f32 / f64 / u16 (depth_kind), rgb [V,H,W,3] u8, keep [V,H,W] u8 or NULL (an object mask,
 *   a depth truncation of the caller's), K [V,3,3] f64 row-major.  z = (double)depth / depth_scale (depth_scale > 0; 1.0 for metres).
 *   rows [V*H*W, 6] f32, row = pixel in row-major order (u = column, v = line): xyz = the float32 cast of the float64 values
 *   x = ((u - K02) * z) / K00, y = ((v - K12) * z) / K11, z (structure/utils.py:465-467, the arithmetic and order of section VP);
 *   flip != 0 negates y and z afterwards (get_pc mode 2, structure/gapartnet.py:576-578); rgb = (float)(u8 / 255.0).
 *   A pixel is VALID when z is finite and > 0 and keep, if given, is non-zero.  DECISION: the reference keeps depth != 0; a negative
 *   or non-finite depth has no meaning for a sensor.  DECISION: a valid depth whose x, y or z overflows float32 is invalid as well,
 *   so that "valid" and "the row's three coordinates are finite" (the rule of section CP) are one set.  The xyz of an invalid pixel
 *   is NaN (all three) - what gpn_cloud_pack, gpn_cloud_finish and gpn_cloud_nearest treat as "no point"; its rgb is written.
 *   valid [V,H,W] u8 = 1 / 0 and valid_counts [V] i32 stay on the device.
 * gpn_frame_select: the seeded presample (the reference's random.sample(range(N), 4 * sampled_num), structure/gapartnet.py:596-601,
 *   which draws from Python's global generator and cannot be repeated) and the compaction.  DECISION: a counter-based rule, a pure
 *   function of (seed, pixel).  seeds [V] u32.  With uint32 arithmetic that wraps,
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     h = mix(mix(pixel + seed * 0x9E3779B9) ^ seed),   hq = h >> (32 - hash_bits)   (hash_bits 1 .. 32; callers pass 32)
 *   a frame with more than cap valid pixels keeps the cap pixels with the smallest 64-bit key (hq << 32) | pixel - the keys are
 *   unique, so is the set; a frame with at most cap valid pixels keeps all of them; cap == 0 keeps every valid pixel of every frame.
 *   How: a radix select of the cap-th smallest hq, 8 bits a pass, the digit histograms built in LDS and merged into the frame's
 *   by integer adds; the threshold t and the number r of pixels with hq == t to admit (lowest pixel first) are resolved on the
 *   device; then per-chunk counts (a chunk = 1024 pixels, one workgroup), a scan over the chunks, and ballot-ordered stores.
 *   Outputs in the layout gpn_cloud_pack writes: packed [V, n_bound, 4] f32 = the rows' .xyz and .w = 1e10, n_bound = cap (H*W when
 *   cap == 0); counts [V] i32 = min(valid, cap); status [V] i32 = GPN_CLOUD_OK or GPN_CLOUD_EMPTY; pix [V, H*W] i32 = the kept
 *   pixels' linear indices, ascending (the first counts[v] entries are written).  DECISION: pix has the pitch H*W, not n_bound:
 *   gpn_cloud_finish clamps the row indices it reads to the n_bound it is given, so it takes (pix, n_bound = H*W) while gpn_view_fps
 *   takes (packed, n_bound = cap); with that, gpn_view_fps, gpn_cloud_finish and gpn_cloud_nearest run unchanged on offsets[v] =
 *   v * H*W.  cap == 0 equals gpn_cloud_pack on the same rows bit for bit.
 * ================================================================================================ */
#define GPN_FRAME_DEPTH_F32 0
#define GPN_FRAME_DEPTH_F64 1
#define GPN_FRAME_DEPTH_U16 2
int gpn_frame_backproject(const void* depth, int depth_kind, double depth_scale, const uint8_t* rgb, const uint8_t* keep,
                          const double* K, int V, int H, int W, int flip, float* rows, uint8_t* valid, int32_t* valid_counts,
                          gpn_stream_t stream);
size_t gpn_frame_select_ws_bytes(int V, int H, int W);
int gpn_frame_select(const float* rows, const uint8_t* valid, const int32_t* valid_counts, const uint32_t* seeds, int V, int H, int W,
                     int cap, int hash_bits, int64_t n_bound, float* packed, int32_t* pix, int32_t* counts, int32_t* status, void* ws,
                     size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * GS - an opt-in sampler for inference that is not sequential: octree cells instead of furthest point sampling.  It fills the slot
 * of gpn_view_fps between gpn_cloud_pack / gpn_frame_select and gpn_cloud_finish; its cost is one sort and a few passes over the
 * rows.  DECISION: opt-in only.  The checkpoints were trained on FPS-sampled clouds, so FPS stays the default of every entry point
 * and the converter (section VP) is not touched: training data stays what the reference produces.  No host read between the
 * launches; no float atomics; integer atomics only where order cannot matter (min / max by integer compare, histograms,
 * counters); every output is bit-reproducible and a pure function of the cloud's rows and its seed - not of the other clouds of
 * the call, of launch order or of the grid size.
 * packed [S, n_bound, 4] f32, counts [S] i32 and status [S] i32 are what gpn_cloud_pack / gpn_frame_select write (S <= 65535,
 * S * n_bound < 2^31); packed is NOT written (gpn_view_fps overwrites .w).  seeds [S] u32; hash_bits 1 .. 32 (callers pass 32; small
 * values force hash ties in tests, as in section FR).  idx [S, m] i32 = packed row indices, read by gpn_cloud_finish as it reads
 * FPS's; level [S] i32 = the octree level L* that was used, -1 where nothing was sampled.
 * Per cloud with status GPN_CLOUD_OK and n = counts[s]: n < m sets GPN_CLOUD_FEW, leaves idx untouched, level = -1 (the rule of
 * gpn_view_fps); n == m gives idx = 0 .. m-1, level = -1; a cloud whose status is not OK is skipped (level = -1); n > m is sampled
 * (j = the packed index of a row, p its xyz):
 *   1. lo_a, hi_a = the fp32 min and max per axis over the n rows; e = the largest of the three fp32 differences hi_a - lo_a.
 *   2. e > 0 and finite: s = (float)(1024.0 / (double)e), q_a = (uint32)min((p_a - lo_a) * s, 1023.0f) - the subtraction and the
 *      product one fp32 operation each, the cast truncating.  Otherwise (all points equal, an overflowing extent) every q_a = 0.
 *      DECISION: min(x, 1023) is "x if x < 1023 else 1023": an extent so small that s overflows to +inf gives 0 * inf = NaN on
 *      the rows at lo_a, which therefore land in cell 1023 with all the others of that axis.
 *   3. code = the 30-bit Morton code, bit 3i + a of code = bit i of q_a (a = 0, 1, 2 for x, y, z).  The point's key is
 *      (uint64)code << 32 | j; its level-L cell is code >> (30 - 3L), L = 0 .. 10.
 *   4. C_L = the number of occupied level-L cells (C_0 = 1).  L* = the largest L with C_L <= m.
 *   5. Stage A: every occupied level-L* cell contributes its point of smallest key.  r = m - C_L*.
 *   6. Stage B (r > 0), with hq(v) = mix(mix(v + seed * 0x9E3779B9) ^ seed) >> (32 - hash_bits), the hash of section FR:
 *      L* < 10: of the occupied level-(L*+1) cells that hold no stage-A point (C_{L*+1} - C_L* > r of them) the r with the smallest
 *      (uint64)hq(cell) << 32 | cell, each contributing its point of smallest key.  L* == 10: of the points stage A did not take
 *      the r with the smallest (uint64)hq(j) << 32 | j.
 *   7. idx[s, :] = the m chosen packed indices in ASCENDING order; level[s] = L*.
 *   Every point shares a level-L* cell (edge e / 2^L*) with a stage-A sample: the coverage radius is at most sqrt(3) e / 2^L*
 *   plus the quantisation slack.  DECISION: 10 bits an axis and no more.  A cloud whose extent is dominated by a few far outliers
 *   fills few cells per level, reaches L* == 10 with C_10 <= m and degrades into the hashed fill of that branch - a uniform
 *   random subset of the points stage A left, no worse than the presample of section FR.
 * How: the workgroups of a cloud share it in chunks of 1024 rows, as in section FR.  Bounds by integer atomicMin / atomicMax on
 * the order-preserving integer image of the floats; ONE stable rocprim::radix_sort_pairs over the keys (cloud, dead, code) of all
 * S * n_bound rows with the row index as payload - a cloud's live rows come out first in its own segment, ordered by (code, j);
 * adjacent sorted codes give, per row, the first level at which it opens a new cell, and a 12-bin histogram of that gives all
 * eleven C_L.  DECISION: the stage-A point of a cell is the first row of the cell in sorted order, and a level-(L*+1) cell holds
 * no stage-A point exactly when its first row opens a cell at level L*+1 and not at L* - both read off the same per-row level.
 * Stage B's r-th smallest hash is the radix select of gpn_frame_select (8 bits a pass, LDS histograms, threshold and tie count
 * resolved on the device; ties admitted in ascending cell / row order).  The output is a flag per row, per-chunk counts and
 * ballot-ordered stores, not a second sort.
 * gpn_cloud_grid_sample_ws_bytes(S, n_bound): the workspace, 0 for S <= 0 or n_bound <= 0.  Errors (GPN_ERR_ARG, nothing
 * launched): m < 1, hash_bits outside 1 .. 32, S > 65535, S * n_bound >= 2^31, a null pointer, a workspace smaller than that.
 * ================================================================================================ */
size_t gpn_cloud_grid_sample_ws_bytes(int S, int64_t n_bound);
int gpn_cloud_grid_sample(const float* packed, int64_t n_bound, const int32_t* counts, int32_t* status, const uint32_t* seeds, int S,
                          int m, int hash_bits, int32_t* idx, int32_t* level, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * OB - object isolation: the `keep` mask of gpn_frame_backproject from the raw frame itself, by classical geometry - seeded RANSAC
 * planes (the table, a wall), the cut at them, connected components of what is left in image space, the object's component.  The
 * reference takes this mask from Grounded-SAM (seg_obj -> obj_mask, structure/gapartnet.py:742-749), which is out of scope here.
 * The rules of section FR hold: a batch of V frames of one size H x W (V <= 65535; here also H, W <= 16384); no host read between
 * the launches; no float atomics; integer atomics only where their order cannot matter (counters, min / max by integer compare);
 * every output is bit-reproducible and independent of what else is in the batch.  The library is built with -ffp-contract=off:
 * every float64 expression below is evaluated as written, one rounding per operation, so numpy gives the same bits.
 * Inputs: rows [V*H*W, 6] f32, valid [V,H,W] u8 and valid_counts [V] i32 of gpn_frame_backproject; pix [V, H*W] i32 of
 * gpn_frame_select with cap == 0 (the valid pixels, ascending); seeds [V] u32.  (x, y, z) of a pixel are its row's first three
 * floats cast to float64.  flip frames work unchanged: the camera is at the origin either way, and "depth" means |z|.
 * A plane is (nx, ny, nz, d) f64 with |n| = 1 and d > 0 - the camera on the positive side; dist(p) = ((nx*x + ny*y) + nz*z) + d.
 * gpn_frame_candidates: cand [V,H,W] u8 = valid && z_min <= |z| <= z_max (z_min >= 0; z_max may be +inf).  cand is the state of
 *   the rounds: gpn_frame_plane_cut clears bytes of it.
 * gpn_frame_plane_hypotheses (stage 1): hyp [V, n_hyp, 4] f64, 1 <= n_hyp <= GPN_ISOLATE_MAX_HYP; hyp_pix [V, n_hyp] i32 = the
 *   pixel of the hypothesis' first point p0, -1 where degenerate.  Point j = 0, 1, 2 of hypothesis k in round r has the counter
 *   c = 3 * n_hyp * r + 3 k + j.  DECISION: a round draws from pix (all valid pixels) and REDRAWS a pixel that is no candidate any
 *   more, rather than compacting the candidates again: try t = 0 .. GPN_ISOLATE_TRIES - 1 takes the rank
 *   hash(seed_v, c + t * 3 * n_hyp * GPN_ISOLATE_MAX_PLANES) mod valid_counts[v] (uint32 arithmetic that wraps; hash = the
 *   mix(mix(i + seed * 0x9E3779B9) ^ seed) of section FR), and the first try whose pixel pix[v, rank] is a candidate is taken;
 *   none: the hypothesis is degenerate.  The tries' counters lie beyond every round's first tries.  With cand == valid the first
 *   try always hits.  With p0, p1, p2 the three points, e1 = p1 - p0, e2 = p2 - p0:
 *     m = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);  mm = (mx*mx + my*my) + mz*mz;  |e|^2 summed the same way
 *     n = m / sqrt(mm) (each component divided);  d = -((nx*p0x + ny*p0y) + nz*p0z);  d < 0: n = -n, d = -d
 *   Degenerate (all four NaN, scores 0): two of the three ranks coincide; not mm > 1e-12 * (|e1|^2 * |e2|^2); d == 0;
 *   valid_counts[v] < 3; a point with no candidate in GPN_ISOLATE_TRIES tries.
 * gpn_frame_plane_score (stage 2): counts [V, n_hyp] i32 = the number of candidates with |dist(p)| <= tol (tol >= 0, finite, in
 *   the rows' units); zeroed by the call.  variant 0: a workgroup per 1024-pixel chunk, the chunk's candidates in LDS as float64, a
 *   thread per hypothesis walking them, one integer atomicAdd per hypothesis and workgroup; variant 1: pixels in registers, ballot
 *   and popcount per hypothesis (kept for tools/isolate_bench.py).  The counts are the same.
 * gpn_frame_plane_winner: winner [V] i32 = the k of the largest count, ties to the lowest k; -1 when every count is 0.
 * gpn_frame_plane_refit (stage 3): one least-squares refit on the winner's inliers (candidates with |dist| <= tol under hyp[v,
 *   winner]): with q = p - p0 (p0 = the row of hyp_pix[v, winner]) the sums s = sum q, Q = sum q q^T and the count n, as per-chunk
 *   partials in the workspace (inside a chunk: each thread its 4 pixels in ascending order, a shuffle tree per wave, the waves in
 *   order) added up in chunk order; mean = p0 + s / n; C = Q - s s^T / n (C_ab = Q_ab - s_a * s_b / n); the plane's normal is the
 *   singular vector of C's smallest singular value (svd3, pose_math.h), normalised again; d = -((nx*meanx + ny*meany) + nz*meanz),
 *   oriented as in stage 1.  The refit's own inliers i (candidates with |dist| <= tol under it) are counted, and the plane is
 *   ACCEPTED when i >= 3 and (double)i >= min_plane_fraction * (double)(the frame's candidates) (0 <= min_plane_fraction <= 1).
 *   planes [V, max_planes, 4] f64: entry `round` = the plane, NaN when not accepted (no winner, fewer than 3 inliers, d == 0
 *   included); plane_inliers [V, max_planes] i32 = i or 0; n_planes [V] i32 = the accepted rounds so far (round 0 sets it).
 *   1 <= max_planes <= GPN_ISOLATE_MAX_PLANES, 0 <= round < max_planes.
 * gpn_frame_plane_cut (stage 4): under an accepted planes[v, round] a candidate stays one iff dist(p) > tol - strictly on the
 *   camera's side and off the plane; the table, the wall behind the object and what the sensor sees "through" them go.  A round
 *   that was not accepted leaves cand untouched.  The host loops stages 1 - 4 over the rounds; nothing is read back.
 * gpn_frame_components (stage 5): connected components of the candidates under 4-connectivity; two neighbours are linked iff both
 *   are candidates and |za - zb| <= jump_abs + jump_rel * min(za, zb), z = |rows.z| in float64 - flying pixels at depth edges fall
 *   apart into crumbs.  labels [V,H,W] i32 = the SMALLEST linear pixel index of the pixel's component, -1 for a non-candidate - a
 *   unique result; sizes [V, H*W] i32 = the component's pixels at its root (label) pixel, 0 elsewhere; n_components [V] i32 = the
 *   components of at least min_pixels (>= 1) pixels.  How: union-find with the parent array in labels.  16 x 16 tiles in LDS, the
 *   links across tile borders by atomicMin on the global array, then every pixel takes its root.  A root only ever takes a smaller
 *   parent, parent[i] <= i holds at every moment, so every find walk ends by construction; no workgroup waits for another (no grid
 *   barrier, no cooperative launch, no flag).
 * gpn_frame_component_select (stage 6): select = GPN_ISOLATE_SELECT_LARGEST: the component with the most pixels, ties to the
 *   smallest root; _CENTER: the component that holds the candidate pixel nearest the anchor (anchor [V,2] i32 = column, line; each
 *   clamped to [-16384, 32767]) by the integer squared pixel distance, ties to the smallest pixel index; _ALL: every component.
 *   DECISION: under all three rules only components of at least min_pixels pixels count (the reference's "magic number" 6 for a
 *   usable mask, structure/gapartnet.py:635), so a frame of crumbs is EMPTY under "largest" too.  keep [V,H,W] u8; chosen [V] i32
 *   = the root (_ALL: the largest's), -1 when none; status [V] i32 = GPN_ISOLATE_EMPTY (no component qualifies, keep all zero),
 *   else GPN_ISOLATE_NO_PLANE (n_planes[v] == 0: components are selected all the same), else GPN_ISOLATE_OK.
 * Errors (GPN_ERR_ARG / GPN_ERR_WS, nothing launched): sizes or parameters outside the ranges above, a null pointer with V > 0,
 * a workspace smaller than the _ws_bytes of the call.  V == 0 returns GPN_OK.
 * Out of scope: learned segmentation, scenes of several objects beyond _ALL, temporal smoothing.
 * ================================================================================================ */
#define GPN_ISOLATE_OK 0
#define GPN_ISOLATE_NO_PLANE 1
#define GPN_ISOLATE_EMPTY 2
#define GPN_ISOLATE_SELECT_LARGEST 0
#define GPN_ISOLATE_SELECT_CENTER 1
#define GPN_ISOLATE_SELECT_ALL 2
#define GPN_ISOLATE_MAX_PLANES 4
#define GPN_ISOLATE_MAX_HYP 1024
#define GPN_ISOLATE_TRIES 8
int gpn_frame_candidates(const float* rows, const uint8_t* valid, int V, int H, int W, double z_min, double z_max, uint8_t* cand,
                         gpn_stream_t stream);
int gpn_frame_plane_hypotheses(const float* rows, const uint8_t* cand, const int32_t* pix, const int32_t* valid_counts,
                               const uint32_t* seeds, int V, int H, int W, int n_hyp, int round, double* hyp, int32_t* hyp_pix,
                               gpn_stream_t stream);
int gpn_frame_plane_score(const float* rows, const uint8_t* cand, const double* hyp, int V, int H, int W, int n_hyp, double tol,
                          int variant, int32_t* counts, gpn_stream_t stream);
int gpn_frame_plane_winner(const int32_t* counts, int V, int n_hyp, int32_t* winner, gpn_stream_t stream);
size_t gpn_frame_plane_refit_ws_bytes(int V, int H, int W);
int gpn_frame_plane_refit(const float* rows, const uint8_t* cand, const double* hyp, const int32_t* hyp_pix, const int32_t* winner,
                          int V, int H, int W, int n_hyp, double tol, double min_plane_fraction, int round, int max_planes,
                          double* planes, int32_t* plane_inliers, int32_t* n_planes, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_frame_plane_cut(const float* rows, const double* planes, int V, int H, int W, int max_planes, int round, double tol,
                        uint8_t* cand, gpn_stream_t stream);
int gpn_frame_components(const float* rows, const uint8_t* cand, int V, int H, int W, double jump_abs, double jump_rel, int min_pixels,
                         int32_t* labels, int32_t* sizes, int32_t* n_components, gpn_stream_t stream);
size_t gpn_frame_component_select_ws_bytes(int V);
int gpn_frame_component_select(const int32_t* labels, const int32_t* sizes, const int32_t* n_planes, const int32_t* anchor, int V,
                               int H, int W, int select, int min_pixels, uint8_t* keep, int32_t* chosen, int32_t* status, void* ws,
                               size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * RD - articulated assets -> training views (the reference's dataset/render_tools/render.py without SAPIEN): z-depth, the winning
 * triangle, link labels, the NPCS map and a flat-shaded RGB image for a batch of V views of one size H x W (H, W <= 16384, V <=
 * 65535).  Views may show different assets.  No host read between the launches; no float atomics; every pixel is stored once, so
 * the images do not depend on launch order.  All float64 arithmetic is uncontracted and in the order written here.
 * Geometry, uploaded once per asset set: verts [Nv,3] f32 as parsed, tris [Nt,3] i32 (rows of verts), tri_visual [Nt] i32 and
 *   tri_link [Nt] i32 (the visual / link of the triangle, counted inside its asset), tri_color [Nt,3] f32 in [0,1],
 *   assets [A,4] i32 = (first triangle, triangle count, visual count, link count).  DECISION: links are numbered inside their
 *   asset because every per-link table below is per view, so the table needs no first-link column.
 * Per view: view_asset [V] i32; cam [V,20] f64 = fx fy cx cy | R [3,3] row-major = meta world2camera_rotation | t [3] = meta
 *   camera2world_translation | the light direction in the camera frame [3] (unit) | pad; vis_mat [V,M,3,4] f64 = world-to-camera
 *   * link pose * visual origin of every visual (composed on the host), camera point = ((m0 x + m1 y) + m2 z) + m3 per row;
 *   link_cat [V,L] i32 (category id, -1 for a link that is no target), link_rank [V,L] i32 (position in the annotation file),
 *   link_frame [V,L,13] f64 = T [3] | scaler | R [3,3] row-major, the NPCS frame of get_NPCS_map_from_oriented_bbox.
 * DECISION: pixel (x, y) samples the ray through u = x, v = y - the ray the reference's own back-projection (x - cx) z / fx
 *   assumes, so back-projected points lie on the mesh.
 * gpn_render_setup, one thread per (view, triangle): u = (fx X) / Z + cx, v = (fy Y) / Z + cy, snapped to rint(u * 256) (half to
 *   even), 1 / Z kept as f64; the triangle is oriented to positive doubled area in int64 (no back-face culling: PartNet meshes are
 *   not consistently wound).  Dropped and counted in counters [V, GPN_RENDER_COUNTERS] i32 (zeroed here), first rule that applies:
 *   an index outside its table (DROP_INDEX); any vertex with Z < 0.1 or NaN (DROP_NEAR; DECISION: the whole triangle goes, cameras
 *   sit 3.5 to 4.5 units away); a snapped coordinate outside +-16384 px (DROP_GUARD); zero doubled area (DROP_ZERO_AREA); a pixel
 *   box that holds no pixel centre of the image (DROP_OFFSCREEN).  Writes one 64-byte record (snapped vertices, three 1 / Z, shade, clipped pixel
 *   box) and one 8-byte box per (view, triangle slot) into the workspace; Nt_max = the largest triangle count of a view's asset.
 * gpn_render_raster, one 256-lane workgroup per 16 x 16 tile per view, one pixel per lane: the boxes are scanned in chunks of 256,
 *   hits are compacted in triangle order into LDS by wave ballots, then every lane walks the list.  Coverage: int64 edge
 *   functions E(a,b,p) = (bx - ax)(py - ay) - (by - ay)(px - ax) at p = (256 x, 256 y), all >= 0, an E == 0 edge counts only when
 *   it runs up (dy < 0) or level to the right (dy == 0, dx > 0) - the top-left rule: a shared edge belongs to one triangle.
 *   li = (double)Ei / (double)(E0 + E1 + E2), invz = (l0 iz0 + l1 iz1) + l2 iz2, winner = largest invz, ties to the lowest
 *   triangle.  depth [V,H,W] f32 = (float)(1 / invz), 0 where empty; tri [V,H,W] i32 = row of tris, -1 where empty.
 * gpn_render_annotate: link_area [V,L] i32 = pixels won per link; link_inst [V,L] i32 = 0, 1, ... in link_rank order over the
 *   target links with area > 0, -1 otherwise (render_sem_ins_seg_map's part_ins_cnt loop); sem / ins [V,H,W] i32 = -2 where |depth|
 *   < 1e-6, -1 on a non-target link, else category / instance id; npcs [V,H,W,3] f32 where ins >= 0, else 0: pc = (((x - cx) z)
 *   / fx, ((y - cy) z) / fy, z) with z = (double)depth, w_r = ((pc0 R[r][0] + pc1 R[r][1]) + pc2 R[r][2]) + t_r, g = (w - T) /
 *   scaler, npcs_r = (float)((g0 Rl[r][0] + g1 Rl[r][1]) + g2 Rl[r][2]); rgb [V,H,W,3] u8 = the background where empty, else
 *   clip(rint((colour * shade) * 255)), shade = 0.5 + 0.5 |n . l| / |n| with n the float64 camera-space cross product (v1 - v0) x
 *   (v2 - v0).  RGB is an approximation of the reference's renderer (no textures, point lights or shadows), not a contract.
 * L <= gpn_render_max_links().  V == 0 and Nt_max == 0 are valid (empty images).
 * ================================================================================================ */
#define GPN_RENDER_COUNTERS 5
#define GPN_RENDER_DROP_INDEX 0
#define GPN_RENDER_DROP_NEAR 1
#define GPN_RENDER_DROP_GUARD 2
#define GPN_RENDER_DROP_ZERO_AREA 3
#define GPN_RENDER_DROP_OFFSCREEN 4
int gpn_render_max_links(void);
size_t gpn_render_ws_bytes(int V, int Nt_max);
int gpn_render_setup(const float* verts, int Nv, const int32_t* tris, const int32_t* tri_visual, int Nt, const int32_t* assets,
                     int A, const int32_t* view_asset, const double* cam, const double* vis_mat, int M, int V, int H, int W,
                     int Nt_max, void* ws, size_t ws_bytes, int32_t* counters, gpn_stream_t stream);
int gpn_render_raster(const int32_t* assets, int A, const int32_t* view_asset, int Nt, int V, int H, int W, int Nt_max,
                      const void* ws, size_t ws_bytes, float* depth, int32_t* tri, gpn_stream_t stream);
int gpn_render_annotate(const float* depth, const int32_t* tri, const int32_t* tri_link, const float* tri_color, int Nt,
                        const int32_t* assets, int A, const int32_t* view_asset, const double* cam, const int32_t* link_cat,
                        const int32_t* link_rank, const double* link_frame, int L, int V, int H, int W, int Nt_max, const void* ws,
                        size_t ws_bytes, int bg_r, int bg_g, int bg_b, int32_t* link_area, int32_t* link_inst, int32_t* sem,
                        int32_t* ins, float* npcs, uint8_t* rgb, gpn_stream_t stream);

/* ================================================================================================
 * RS - textured, lit RGB for the views of section RD (shading = "textured"): one launch after gpn_render_annotate that overwrites
 * the rgb field and nothing else.  One 256-lane workgroup per 16 x 16 tile per view, one pixel per lane; the view's light rows
 * are read once per workgroup into LDS; no atomics, no workspace, every output byte is written exactly once.  Everything is
 * float64 in the order written here and uses only + - * / sqrt floor rint, so a host restatement agrees to the byte.
 * Extra geometry: tri_uv [Nt,3,2] f32 = the vt of each corner in parsed corner order (NaN where a corner has none); tri_tex [Nt]
 *   i32 = row of tex_table, -1 for none; tex_table [T,4] i32 = (first texel, w, h, 0); tex_data [texels] u32, a texel is the bytes
 *   r g b 255 in memory order (r = bits 0-7); texels < 2^31.  T == 0: tri_uv, tri_tex, tex_table and tex_data are not read.
 * Per view: lights [V,NL,8] f64 in the camera frame of the view, NL <= gpn_render_max_lights() = 16; a row is kind | x y z | r g b
 *   | pad.  Kind 0 ambient; kind 1 directional, x y z = the unit vector TOWARDS the light; kind 2 point, x y z = its position.
 *   Rows of another kind are skipped.
 * For pixel (x, y) of view v with t = tri[v,y,x] inside the view's asset (otherwise: the background colour):
 *   corners: P[3] (camera space, parsed order) and the snapped screen corners exactly as gpn_render_setup computes them (one
 *     shared device function); flip = the doubled area of the parsed order is negative, oriented corners (0,1,2) or (0,2,1).
 *   barycentrics: E0, E1, E2 = the raster's edge functions at (256 x, 256 y) over the oriented corners, l_j = (double)E_j /
 *     (double)((E0 + E1) + E2), w_j = l_j * (1 / Z_j), b_j = w_j / ((w0 + w1) + w2); b is mapped back to parsed order.
 *   uv = (b0 uv0 + b1 uv1) + b2 uv2, each corner's f32 widened first.
 *   albedo_c in 0 ... 255: (double)tri_color[t][c] * 255, unless tri_tex[t] names a texture and all six tri_uv values are finite:
 *     u' = u - floor(u), v' = (1 - v) - floor(1 - v) (OBJ origin bottom-left, row 0 of the image is its top); X = u' w - 0.5,
 *     i = floor(X), fx = X - i; Y = v' h - 0.5, k = floor(Y), fy = Y - k; columns i mod w and (i + 1) mod w, rows k mod h and
 *     (k + 1) mod h (wrapping: i = -1 is w - 1); albedo_c = (a00 (1 - fx) + a01 fx)(1 - fy) + (a10 (1 - fx) + a11 fx) fy with
 *     a[row][column].  A tri_tex outside [-1, T) or a table row whose span leaves tex_data counts as no texture.
 *   normal: n = (P1 - P0) x (P2 - P0), nn = sqrt((nx nx + ny ny) + nz nz), n = n / nn, negated when (nx P0x + ny P0y) + nz P0z >
 *     0 (two-sided, towards the camera).  nn == 0: only the ambient rows count.
 *   pixel point: z = (double)depth, p = (((x - cx) z) / fx, ((y - cy) z) / fy, z) as in gpn_render_annotate.
 *   intensity, rows in table order, I_c = 0 first: ambient I_c = I_c + col_c; directional m = max(0, (nx dx + ny dy) + nz dz),
 *     I_c = I_c + col_c m; point D = L - p, r2 = (Dx Dx + Dy Dy) + Dz Dz, r = sqrt(r2), skipped when r == 0, m = max(0, ((nx Dx +
 *     ny Dy) + nz Dz) / r), I_c = I_c + (col_c m) / r2.
 *   rgb_c = rint(albedo_c * I_c) clamped to 0 ... 255.
 * The tables live on the device, so the entry point checks what it can see (null pointers, NL, T, texels, sizes); the contents
 * of tri_tex and tex_table are bounds-checked in the kernel (never a fault) and refused by the Python layer before the upload.
 * ================================================================================================ */
int gpn_render_max_lights(void);
int gpn_render_shade(const float* verts, int Nv, const int32_t* tris, const int32_t* tri_visual, const float* tri_color, int Nt,
                     const int32_t* assets, int A, const int32_t* view_asset, const double* cam, const double* vis_mat, int M,
                     const float* tri_uv, const int32_t* tri_tex, const int32_t* tex_table, int T, const void* tex_data,
                     int64_t texels, const double* lights, int NL, const float* depth, const int32_t* tri, int V, int H, int W,
                     int Nt_max, int bg_r, int bg_g, int bg_b, uint8_t* rgb, gpn_stream_t stream);

/* ================================================================================================
 * PF - pose fitting.  replaces the per-proposal numpy loop of gapartnet/misc/pose_fitting.py:4-147 (estimate_pose_from_npcs:
 * 5-point RANSAC over Umeyama similarity fits, Umeyama on the inliers, NPCS-aligned box; callers network/model.py:966-980,
 * structure/utils.py:172-188) for ALL proposals of a batch: two launches, float64 like the reference.
 * xyz / npcs [M,3] f64 (proposal p = rows offsets[p]:offsets[p+1], non-empty), picks [P,H,5] i64 = the reference's
 * np.random.randint(n, size=5) draws per iteration (drawn by the caller: gapartnet_amd.misc.pose_fitting_batched.draw_picks).
 * outputs: valid [P] u8, scale [P], rotation [P,3,3], translation [P,3], transform [P,4,4], bbox [P,8,3] (NaN where not
 * valid), inlier_mask [M] u8, best_iteration [P] i64, residual [P,H] (of every hypothesis, as the reference computes it).
 * ================================================================================================ */
size_t gpn_pose_fit_ws_bytes(int64_t P, int H);
int gpn_pose_fit(const double* xyz, const double* npcs, const int64_t* offsets, const int64_t* picks, int64_t P, int64_t M,
                 int H, double stop_thrsh, uint8_t* valid, double* scale, double* rotation, double* translation,
                 double* transform, double* bbox, uint8_t* inlier_mask, int64_t* best_iteration, double* residual, void* ws,
                 size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * JE - joint estimation: the axis direction, a point on the axis and the angle of the joint a part moved about, from two
 * observations of the part (the reference's estimate_joint_angle, structure/gapartnet.py:819-963), for a batch of B pairs.
 * Three launches, float64 like the reference, no host read between them, no float atomics: every reduction has a fixed shape
 * (per-thread strided sums, a shuffle tree per wave, the waves in order), so results are bit-reproducible and a pair's result
 * does not depend on the other pairs of the batch.  K <= GPN_JOINT_MAX_K.
 * gpn_joint_sample (:836-845): pc1 [n1_total,3], pc2 [n2_total,3] f64, pair b = rows off[b]:off[b+1] (off1, off2 [B+1] i64);
 *   picks1, picks2 [B,K] i64 = rows INSIDE the pair's segment (the reference's random.sample; drawn by the caller:
 *   gapartnet_amd.misc.joint_fitting.draw_joint_picks); k1, k2 [B] i32 = live picks of the row.  M = mean of the pair's pc2
 *   rows, S = the largest per-axis extent max(pc2 - M) - min(pc2 - M), X = (pc1[picks1] - M) / S, Y = (pc2[picks2] - M) / S (a
 *   division).  X, Y [B,K,3], rows beyond k zero; norm [B,4] = (S, Mx, My, Mz).  An empty pc2 segment gives NaN; a pick outside
 *   its segment gives a NaN row and reads nothing.
 * gpn_cpd_rigid: Coherent Point Drift rigid registration (Myronenko & Song 2010, as pycpd.RigidRegistration runs it with its
 *   defaults) of the moving set Y [B,K,3] (M = ny[b] rows) onto the fixed set X [B,K,3] (N = nx[b] rows), one workgroup a pair,
 *   the whole EM loop in the launch.  Row convention: TY = s Y R + t.
 *   Start: R = I, t = 0, s = 1, sigma2 = sum_mn |x_n - y_m|^2 / (3 M N), q = diff = inf.
 *   While iteration < max_iterations and diff > tolerance (a NaN diff ends the loop):
 *     E: P_mn = exp(-|x_n - TY_m|^2 / (2 sigma2)) / den_n, den_n = max(sum_m exp(..), DBL_EPSILON) + c,
 *        c = (2 pi sigma2)^(3/2) w / (1 - w) M / N (no column maximum is subtracted first).
 *     M: Np = sum P, muX = sum_n Pt1_n x_n / Np, muY = sum_m P1_m y_m / Np, A = sum_mn P_mn (x_n - muX)(y_m - muY)^T = U S V^T,
 *        R = (U diag(1, 1, det(U V^T)) V^T)^T, YPY = sum_m P1_m |y_m - muY|^2, s = tr(A R) / YPY (1 when scale == 0),
 *        t = muX - s R^T muY, TY = s Y R + t.
 *     Variance: xPx = sum_n Pt1_n |x_n - muX|^2, q' = (xPx - 2 s tr(A R) + s^2 YPY) / (2 sigma2) + 1.5 Np ln sigma2,
 *        diff = |q' - q|, sigma2 = (xPx - s tr(A R)) / (3 Np), replaced by tolerance / 10 when <= 0.
 *   The M x N matrix is never stored: every sum above is a sum over columns n of per-column sums over m.
 *   Outputs: s [B], R [B,3,3], t [B,3], sigma2 [B], q [B], diff [B], iterations [B] i32, and sigma2_trace [B,max_iterations]
 *   or NULL = sigma2 at the end of every iteration run, NaN after the last.  A pair with nx or ny outside 1 .. K writes NaN
 *   and iterations = 0.  0 <= w < 1.
 * gpn_joint_from_rigid (:850-856 = :867-873) for G transforms: rotation [G,3,3], translation [G,3], norm [G,4] ->
 *   axis [G,3], pivot [G,3], angle [G].  GPN_JOINT_REVOLUTE: the rotation vector through the unit quaternion with w >= 0 as
 *   scipy's Rotation.from_matrix(..).as_rotvec(); angle = |rotvec|, axis = rotvec / angle (NaN at angle 0, as in the reference),
 *   r = the matrix of the rotation vector (pi/2 - angle/2) axis, pivot = (t r / 2) / sin(angle / 2) * S + M.
 *   GPN_JOINT_PRISMATIC (an extension: the reference takes joint_type and ignores it): axis = t / |t|, angle = |t| S (the
 *   displacement), pivot = M.
 * ================================================================================================ */
#define GPN_JOINT_MAX_K 4096
#define GPN_JOINT_REVOLUTE 0
#define GPN_JOINT_PRISMATIC 1
int gpn_joint_sample(const double* pc1, const double* pc2, const int64_t* off1, const int64_t* off2, const int64_t* picks1,
                     const int64_t* picks2, const int32_t* k1, const int32_t* k2, int64_t B, int K, double* X, double* Y,
                     double* norm, gpn_stream_t stream);
int gpn_cpd_rigid(const double* X, const double* Y, const int32_t* nx, const int32_t* ny, int64_t B, int K, int max_iterations,
                  double tolerance, double w, int scale, double* s, double* R, double* t, double* sigma2, double* q, double* diff,
                  int32_t* iterations, double* sigma2_trace, gpn_stream_t stream);
int gpn_joint_from_rigid(const double* rotation, const double* translation, const double* norm, int64_t G, int joint_type,
                         double* axis, double* pivot, double* angle, gpn_stream_t stream);

/* ================================================================================================
 * AR - articulation from two frames: the parts of frame A associated with the parts of frame B, and the matched parts' pixels cut
 * out as the ragged clouds gpn_joint_sample reads - what lies between section FR's per-pixel instance maps and section JE, which
 * takes ONE part and asks for its points ("only part, please segment first", structure/gapartnet.py:829).  The reference has no
 * counterpart.  A batch of V frame pairs of one size H x W (V <= 65535, H and W <= 16384), at most GPN_PARTS_MAX parts a frame.
 * No host read inside an entry point; no float atomics; integer atomics only on histograms, whose results do not depend on their
 * order: every output is bit-reproducible and a frame pair's result does not depend on the rest of the batch.  V == 0 is a valid
 * call that launches nothing, and so is gpn_parts_overlap with both table widths 0 and gpn_parts_gather with P == 0 or n_total == 0;
 * a single width of 0 is valid too (the tables of that side are empty; gpn_parts_match still writes n_matched = 0).
 * MEMBERSHIP, the rule of all three entry points: pixel q of frame v belongs to part p iff valid[v,q] != 0 and inst[v,q] == p with
 *   0 <= p < n_parts[v].  Any other value of inst (-1, a value at or above n_parts[v], a large negative one) belongs to no part.
 *   inst [V,H,W] i32; valid [V,H,W] u8 as gpn_frame_backproject writes it; n_parts [V] i32 on the device (a count above the table
 *   width is read as the table width).
 * gpn_parts_overlap: inter [V,PA,PB] i32 = the pixels that belong to part i in frame A and to part j in frame B; area_a [V,PA],
 *   area_b [V,PB] i32 = the parts' pixels.  PA, PB <= GPN_PARTS_MAX are the table widths; entries at or beyond the live counts
 *   are written as 0.  How: a workgroup per chunk of 1024 pixels (the chunk of section FR) fills a PA x PB histogram in LDS by
 *   integer atomics - a wave first groups its lanes by key with ballots and adds each group's popcount once, since the maps are
 *   piecewise constant - and flushes the non-zero bins by global integer adds.
 * gpn_parts_match: GREEDY one-to-one matching by 2D mask IoU, exact.  cls_a [V,PA], cls_b [V,PB] i32 (either NULL: all classes
 *   equal).  union = area_a[i] + area_b[j] - inter[i,j]; a pair (i, j) is ELIGIBLE iff its classes are equal, inter > 0 and
 *   (double)inter >= min_iou * (double)union (one float64 product and one comparison).  Repeatedly the eligible pair of an
 *   unmatched i and an unmatched j with the largest IoU is taken, until none is left.  IoUs are compared exactly, by the 64-bit
 *   cross products inter1 * union2 and inter2 * union1 (below 2^57 under the frame limits); ties go to the smaller i, then the
 *   smaller j.  DECISION: greedy, not the optimal (Hungarian) assignment - it is the rule this project's AP matching uses, it is
 *   a total order, so the result is unique, and it needs no floating-point cost.  Outputs: match_ab [V,PA] i32 = j or -1,
 *   match_ba [V,PB] i32 = i or -1, n_matched [V] i32, m_inter, m_union [V,PA] i32 (0 where unmatched).  One workgroup a frame
 *   pair: at most 64 rounds of an arg-max over at most 4096 entries held in LDS.
 * gpn_parts_gather: one side's clouds.  rows [V*H*W,6] f32 of gpn_frame_backproject; seg_start [V,P] i64 = the first output row of
 *   the part's segment, or negative to drop the part.  pc [n_total,3] f64: the member pixels of part p of frame v go to rows
 *   seg_start[v,p] + 0, 1, 2, ... in ascending pixel order, xyz cast f32 -> f64 (exact).  Rows no segment covers are not written;
 *   a row at or beyond n_total is not written either.  Segment sizes are the areas of gpn_parts_overlap; overlapping segments are
 *   the caller's error and are not detected.  How: a stable multi-way partition - per-chunk per-part counts, one scan over the
 *   chunks per (frame, part), stores with the in-chunk rank of every pixel among the earlier pixels of its own part (ballots over
 *   equal keys inside a wave, LDS counters added in order across the chunk).  Workspace: gpn_parts_gather_ws_bytes.
 * ================================================================================================ */
#define GPN_PARTS_MAX 64
int gpn_parts_overlap(const int32_t* inst_a, const uint8_t* valid_a, const int32_t* n_a, const int32_t* inst_b,
                      const uint8_t* valid_b, const int32_t* n_b, int V, int H, int W, int PA, int PB, int32_t* inter,
                      int32_t* area_a, int32_t* area_b, gpn_stream_t stream);
int gpn_parts_match(const int32_t* inter, const int32_t* area_a, const int32_t* area_b, const int32_t* n_a, const int32_t* n_b,
                    const int32_t* cls_a, const int32_t* cls_b, double min_iou, int V, int PA, int PB, int32_t* match_ab,
                    int32_t* match_ba, int32_t* n_matched, int32_t* m_inter, int32_t* m_union, gpn_stream_t stream);
size_t gpn_parts_gather_ws_bytes(int V, int H, int W, int P);
int gpn_parts_gather(const float* rows, const int32_t* inst, const uint8_t* valid, const int32_t* n_parts, const int64_t* seg_start,
                     int V, int H, int W, int P, int64_t n_total, double* pc, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * MV - the part predictions of several POSED views of one object fused into object parts: one list of parts in the world frame,
 * every part knowing its mask in every view, its cloud the union of all views' member points (NPCS is canonical per part, so the
 * union is a valid input to gpn_pose_fit).  The reference has no counterpart (ObjIns holds one image); the contract is this
 * project's own.  ONE object per call: V views of one size H x W, 1 <= V <= GPN_VIEWS_MAX (V * H * W < 2^31 - 1024), GT parts over
 * all views, GT <= GPN_FUSE_PARTS_MAX (more is an argument error).  The rules of sections FR and AR hold: no host read inside an
 * entry point; no float atomics; integer atomics only where the result does not depend on their order (minima, histograms,
 * counters); every output is bit-reproducible.  V == 0 and GT == 0 are valid calls that launch nothing or write empty tables (with
 * GT == 0 and V > 0 the per-pixel outputs are still written: no pixel is a member).  Argument errors return 1 without touching the
 * device.
 * INPUT: rows [V*H*W,6] f32 and valid [V,H,W] u8 as gpn_frame_backproject writes them with flip = 0; inst [V,H,W] i32 and n_parts [V]
 *   i32 on the device, MEMBERSHIP exactly as in section AR (a count is read as min(max(n_parts[v], 0), GT)); R [V,3,3], t [V,3]
 *   f64 in the renderer's convention (camera_frame, dataset/render_assets.py): a camera point is (world - t) @ R, so
 *   world = cam @ R^T + t.  GLOBAL PART ID g = base[v] + p with base the exclusive scan of the counts; a part with g >= GT does not
 *   exist (its pixels are members of nothing).
 * gpn_views_world: for every member pixel, in float64, in this order, without fused multiply-add,
 *     w_k = ((x * R[k][0] + y * R[k][1]) + z * R[k][2]) + t[k]      (x, y, z = the float32 row cast up)
 *   wrows [V*H*W,3] f32 = (float)w, NaN (all three) for a non-member pixel; part_of [V,H,W] i32 = g or -1; area [GT] i32 = the member
 *   pixels of each part; lo [3] f64 = (double) of the smallest stored float32 per axis over all member pixels, by atomicMin on the
 *   order-preserving integer image (so -0.0 < +0.0; a member's row is finite whenever R and t are), 0.0 when no pixel is a member.
 * gpn_views_overlap: the occupancy tables on a fixed grid of 1024 cells an axis.  cell > 0 (f64);
 *     i_k = floor(((double)wrows_k - lo_k) / cell)                    (one subtraction, one division)
 *   a member pixel with any i_k outside 0 .. 1023 (or NaN) is DROPPED from the occupancy and counted in dropped [V] i32; it stays a
 *   member for everything else.  vox = i_x << 20 | i_y << 10 | i_z; key = vox << 9 | g, all ones for a non-member or dropped pixel
 *   (keys_out [V*H*W] u64 receives the keys when it is not NULL).  Over the set of distinct (vox, g): vol [GT] i32 = the distinct
 *   voxels of part g; inter [GT,GT] i32, symmetric, zero diagonal: (g, h) = the voxels that hold both g and h, pairs of one view
 *   included.  How: ONE rocprim::radix_sort_keys over 40 bits (the 39 live ones and the bit that puts the all-ones key last),
 *   rocprim::unique, then one lane per distinct entry: vol[g] += 1 and one pair of increments for every LATER entry of its voxel
 *   (a voxel holds at most GT entries).  The pair increments are summed in an LDS table while GT * GT * 4 bytes fit in 64 KiB
 *   (GT <= 128) and flushed by global integer adds, and go to global memory directly above that; gpn_views_overlap_lds_parts(n)
 *   moves that switch (n < 0: query; the bound 128 stays) - both forms give the same tables.  Workspace: gpn_views_overlap_ws_bytes.
 * gpn_views_merge: one workgroup.  cls [GT] i32 (NULL: all equal); view_of[g] from the scan of n_parts (a g beyond the scan's end
 *   has no view and counts as vol == 0).  A pair g < h is ELIGIBLE iff cls[g] == cls[h], inter[g,h] >= max(min_inter, 1),
 *   (double)inter[g,h] >= min_overlap * (double)min(vol[g], vol[h]) (one float64 product, one comparison) and, at the time it is
 *   considered, g and h lie in different clusters whose view sets (one uint64 mask a cluster) are disjoint.  Repeatedly the
 *   eligible pair with the largest inter / min(vol) is taken - compared exactly by the 64-bit cross products (inter < 2^30, so
 *   below 2^60), ties to the smaller g, then the smaller h - its clusters are united and their view masks ORed, until no eligible
 *   pair is left.  Clusters only grow, so a pair refused for its view sets stays refused: the loop equals one pass over the
 *   candidates in that total order, and the result is unique.  DECISION: single linkage, greedy, at most one part per view in a
 *   fused part; normalised by the SMALLER volume, because two views see different faces of one part; not an optimal assignment.
 *   Outputs: fused_of [GT] i32 = fused id 0 .. F-1 in ascending order of each cluster's smallest g, -1 for a part with vol == 0;
 *   n_fused [1] i32 = F; per fused id [GT]: fused_views u64, fused_class i32 (the members' class, 0 with cls == NULL), fused_vol i32
 *   (the sum of the members' vol), fused_parts [GT,V] i32 (the LOCAL part of each view, or -1); links [GT,3] i32 = (g, h, inter) of
 *   every union in the order taken, n_links [1] i32.  Entries at or beyond F: fused_views 0, fused_class -1, fused_vol 0,
 *   fused_parts -1; links at or beyond n_links: (-1, -1, 0).
 * gpn_views_relabel: fused_inst [V,H,W] i32 = fused_of[part_of], or -1: ids consistent across views.
 * gpn_views_gather: npcs [V,H,W,3] f32 (NULL together with npcs_out: none), seg_start [F] i64 = the first output row of fused part f
 *   or negative to drop it, F <= GPN_FUSE_PARTS_MAX.  The pixels with fused_inst == f go to rows seg_start[f] + 0, 1, 2, ... in
 *   ascending (view, pixel) order: xyz [M,3] f64 = the wrows cast up, npcs_out [M,3] f64, src [M] i64 = v * H * W + pixel.  Rows no
 *   segment covers, and rows at or beyond M = n_total, are not written.  How: the stable multi-way partition of gpn_parts_gather
 *   over 9-bit keys, the counts scanned over (view, chunk) per fused part.  Workspace: gpn_views_gather_ws_bytes.
 * ================================================================================================ */
#define GPN_VIEWS_MAX 64
#define GPN_FUSE_PARTS_MAX 512
int gpn_views_world(const float* rows, const uint8_t* valid, const int32_t* inst, const int32_t* n_parts, const double* R,
                    const double* t, int V, int H, int W, int GT, float* wrows, int32_t* part_of, int32_t* area, double* lo,
                    gpn_stream_t stream);
int gpn_views_overlap_lds_parts(int parts);
size_t gpn_views_overlap_ws_bytes(int V, int H, int W);
int gpn_views_overlap(const float* wrows, const int32_t* part_of, const double* lo, double cell, int V, int H, int W, int GT,
                      int32_t* vol, int32_t* inter, int32_t* dropped, uint64_t* keys_out, void* ws, size_t ws_bytes,
                      gpn_stream_t stream);
int gpn_views_merge(const int32_t* inter, const int32_t* vol, const int32_t* cls, const int32_t* n_parts, int V, int GT, int min_inter,
                    double min_overlap, int32_t* fused_of, int32_t* n_fused, uint64_t* fused_views, int32_t* fused_class,
                    int32_t* fused_vol, int32_t* fused_parts, int32_t* links, int32_t* n_links, gpn_stream_t stream);
int gpn_views_relabel(const int32_t* part_of, const int32_t* fused_of, int V, int H, int W, int GT, int32_t* fused_inst,
                      gpn_stream_t stream);
size_t gpn_views_gather_ws_bytes(int V, int H, int W, int F);
int gpn_views_gather(const float* wrows, const float* npcs, const int32_t* fused_inst, const int64_t* seg_start, int V, int H, int W,
                     int F, int64_t n_total, double* xyz, double* npcs_out, int64_t* src, void* ws, size_t ws_bytes,
                     gpn_stream_t stream);

/* ================================================================================================
 * PE - pose evaluation: is an estimated part pose right?  The ground-truth pose of every instance, the exact IoU of two oriented
 * boxes, and the errors of matched (prediction, ground truth) pairs under the part's symmetry group: what the GAPartNet paper
 * reports for its second task (R_e, T_e, S_e, 3D IoU).  The reference has no counterpart (on_test_epoch_end ends at a
 * commented-out "# pose estimation").  Float64 arithmetic, no float atomics, no host read; every reduction has a fixed shape, so
 * results are bit-equal from run to run and one item's result does not depend on the other items of the call.  Counts of 0
 * are valid calls that launch nothing.  Boxes are 8 corners in the order (---, +--, -+-, --+, ++-, +-+, -++, +++) of
 * gpn_pose_fit's bbox.
 * gpn_pose_gt_fit: the similarity xyz ~ npcs @ (s R) + t (row vectors, as gpn_pose_fit) of every ground-truth instance by plain
 *   Umeyama over ALL its points.  xyz, npcs [N,3] f32; slot [N] i32 = scene * W + the point's instance id in its scene, negative =
 *   none (a slot outside its own scene's range is ignored as well); scene_offsets [S+1] i64 on the device.  One workgroup per slot
 *   walks its scene's rows twice (means, then centred moments); the k-th point of an instance always goes to the same thread in the
 *   same turn, whatever lies between the instance's points.  Outputs per slot [S*W]: count i64, valid u8, scale, rotation [3,3],
 *   translation [3], half [3] = max |npcs| per axis over the instance (the observed extent, as gpn_pose_fit's box has it), bbox
 *   [8,3] = (signs * half * s) @ R + t.  valid = 0, with NaN in every float output, for fewer than 3 points, for an NPCS covariance
 *   whose second singular value is below 1e-9 x its first (collinear points) and for non-finite input; a planar instance (rank 2)
 *   is valid: the reflection rule of Umeyama fixes the third axis.
 * gpn_box_iou_3d: IoU of P pairs a [P,8,3], b [P,8,3] f64.  Centre = the corners' mean, axes and half extents from the edges
 *   corner 1, 2, 3 - corner 0.  Each of the 12 faces (6 of a, then 6 of b; face 2 i + 0/1 = the -/+ side of axis i) is clipped by
 *   the 6 half-spaces of the other box (Sutherland-Hodgman, <= 10 vertices) and contributes area * height / 3 with the height from
 *   a's centre along the face's outward normal; intersection = the sum in face order, IoU = inter / (vol a + vol b - inter).
 *   Tie rule: a vertex ON a clipping plane is inside only while a's faces are clipped by b and only if the face's outward normal
 *   and the plane's normal have a positive dot product; otherwise outside.  (Identical boxes then count every shared face once,
 *   touching boxes never.)  ON = a signed distance within 2^-26 x the largest half extent of the two boxes, which is then taken
 *   as 0: an exact test would leave coincident faces of turned boxes to the sign of a rounding error (a box against itself
 *   anywhere between 0.1 and 15).  Accuracy: round-off for boxes in general position; where two faces meet at a small angle a the
 *   intersection points are conditioned like eps / a, so the worst case is about sqrt(eps) ~ 1e-8 near a = 2^-26 rad.
 *   A pair with a non-finite corner or a zero extent gives NaN.
 * gpn_pose_pair_errors for P pairs: (scale [P], rotation [P,3,3], translation [P,3], half [P,3]) of prediction and ground truth,
 *   sym_type [P] i32, and the candidate table sym_table [K,3,3] f64 with sym_start, sym_count [T] i32 per type (count <= 24), all on
 *   the device.  With F_k = S_k R_gt for the type's candidates k in table order:
 *     re_deg = min_k atan2(|v|, (tr M - 1) / 2) in degrees, M = R_pred F_k^T, v = vee of (M - M^T) / 2; k_re = the first minimiser;
 *     te = |t_pred - t_gt|; se = |s_pred - s_gt|;
 *     iou = max_k IoU(box(s_pred, R_pred, t_pred, half_pred), box(s_gt, F_k, t_gt, half_gt)) by the rule above; k_iou = the first
 *     maximiser.  (k counts inside the type: 0 is the type's first candidate.)
 *   Non-finite poses give NaN (and k = 0); a type outside 0 .. T-1 or a table range outside 0 .. K gives NaN and k = -1.
 * ================================================================================================ */
int gpn_pose_gt_fit(const float* xyz, const float* npcs, const int32_t* slot, const int64_t* scene_offsets, int64_t N, int S, int W,
                    int64_t* count, uint8_t* valid, double* scale, double* rotation, double* translation, double* half, double* bbox,
                    gpn_stream_t stream);
int gpn_box_iou_3d(const double* a, const double* b, int64_t P, double* iou, gpn_stream_t stream);
int gpn_pose_pair_errors(const double* scale_pred, const double* rotation_pred, const double* translation_pred, const double* half_pred,
                         const double* scale_gt, const double* rotation_gt, const double* translation_gt, const double* half_gt,
                         const int32_t* sym_type, int64_t P, const double* sym_table, int K, const int32_t* sym_start,
                         const int32_t* sym_count, int T, double* re_deg, int32_t* k_re, double* te, double* se, double* iou,
                         int32_t* k_iou, gpn_stream_t stream);

/* ================================================================================================
 * VS - test-time part predictions and the 3 x 4 panel of images per sampled scene (the reference's on_test_epoch_end,
 * network/model.py:930-999, misc/visu.py, misc/visu_util.py).  Every "the last writer of the loop wins" of the reference is an
 * integer atomicMax over the writer's position and a resolve pass: results are bit-reproducible and never depend on timing; no
 * float atomics; no host read between the launches of an entry point.
 * gpn_scene_maps: one batch's kept proposals -> per-point maps (model.py:954-971).  valid_indices [V] i64 = nonzero(valid_mask),
 *   sorted_indices [M] i64, proposal_offsets [P+1] i64, npcs_valid_mask [M] u8, npcs_preds [Mv,3] f32 (row j belongs to the j-th
 *   true entry of the mask), N rows in the batch.  The row of proposal point m is valid_indices[sorted_indices[m]].
 *   ins_map [N] i32: 0 where no proposal, p + 1 for the points of proposal p; npcs_map [N,3] f32: zero, or the prediction of the
 *   proposal point inside the mask that sits on the row; a row written by several m keeps the highest m (in both maps).
 *   fit_npcs [M,3] f32 = npcs_map at each proposal point, minus 0.5 (a point outside the mask enters the fit as -0.5: kept quirk).
 * gpn_points_winner: the geometry half of map2image (visu_util.py:107-139), once per scene for all its tiles.  xyz [n_total,3] f32
 *   in the normalised frame, scene s = rows scene_offsets[s]:scene_offsets[s+1] (i64 [S+1], on the device), trans [S,4] f64 =
 *   (r, cx, cy, cz) of the meta file.  In float64 without contraction: camera point = double(xyz) * r + c, u = rint(x * fx / z +
 *   u0), v = rint(y * fy / z + v0) (half to even).  A point is dropped if u or v is not finite or v + 1 >= H, v < 0, u + 1 >= W,
 *   u < 0 (-0.0 passes); a kept point covers (v,u), (v+1,u), (v+1,u+1), (v,u+1).  winner [S,H,W] i32 = the highest point index (in
 *   its scene) covering the pixel, -1 where none.
 * gpn_points_paint: all requested tiles of all scenes in one launch, into canvas [S,CH,CW,3] u8; tile (row, col) has its origin at
 *   (edge + row * (H + edge), edge + col * (W + edge)).  A pixel without a winner is white.  Layer kinds (src is indexed by
 *   scene_offsets[s] + winner):
 *     GPN_VISU_RGB            src [n_total,3] f32: u8((src + offset) * 255.0f), float32, truncated toward zero; values outside
 *                             [0, 256) are clamped to [0, 255] and NaN gives 0 (the reference's cast is undefined there)
 *     GPN_VISU_LABEL          src [n_total] i32: palette[floormod(label, K)]
 *     GPN_VISU_LABEL_MOD20    palette[floormod(label, 20)]
 *     GPN_VISU_LABEL_MOD19P1  palette[floormod(label, 19) + 1], label -100 -> (230, 230, 230)
 *     GPN_VISU_BLANK          white everywhere (src unused)
 *   palette [K,3] u8 on the device (K >= 20 for the two modulo rules).
 * gpn_boxes_draw: draw_bbox (visu_util.py:37-71) for all boxes of all scenes into the listed tiles (tiles_host [n_tiles,2] i32 =
 *   (row, col), on the host).  bbox [Q,8,3] f64 in the normalised frame, box_scene [Q] i32.  Corner pixels by the projection rule
 *   above.  The line rule (ours: OpenCV's is not restated): the all-integer Bresenham walk from a to b inclusive - dx = |x1 - x0|,
 *   dy = -|y1 - y0|, err = dx + dy; each step plots the current pixel, stops at b, then with e2 = 2 err: e2 >= dy steps x and adds
 *   dy to err, e2 <= dx steps y and adds dx to err - each plotted pixel stamped as a t x t square whose top-left is (x - t/2,
 *   y - t/2); pixels outside the tile are dropped; an edge with a non-finite endpoint or one outside [-4W, 5W) x [-4H, 5H) is
 *   skipped.  Per box GPN_VISU_BOX_DRAWS draws in the reference's order: the edges 0-1 0-2 0-3 1-4 1-5 2-6 6-3 4-7 5-7 3-5 2-4 6-7
 *   in (255, 0, 255) with t = 2, then 0-1 (255, 0, 0), 0-3 (0, 0, 255), 0-2 (0, 255, 0) with t = 3 (colours as in the written
 *   file).  The result equals drawing box by box and draw by draw in that order: a pixel keeps the highest q * 15 + e.
 * ================================================================================================ */
#define GPN_VISU_RGB 0
#define GPN_VISU_LABEL 1
#define GPN_VISU_LABEL_MOD20 2
#define GPN_VISU_LABEL_MOD19P1 3
#define GPN_VISU_BLANK 4
#define GPN_VISU_MAX_LAYERS 16
#define GPN_VISU_BOX_DRAWS 15
typedef struct {
  int32_t kind;    /* GPN_VISU_* */
  int32_t row;     /* tile row */
  int32_t col;     /* tile column */
  float offset;    /* GPN_VISU_RGB: added before the scale */
  const void* src; /* device pointer, see above */
} gpn_visu_layer_t;
size_t gpn_scene_maps_ws_bytes(int64_t N, int64_t M);
int gpn_scene_maps(const int64_t* valid_indices, int64_t V, const int64_t* sorted_indices, const int64_t* proposal_offsets,
                   int64_t P, const uint8_t* npcs_valid_mask, int64_t M, const float* npcs_preds, int64_t Mv, int64_t N,
                   int32_t* ins_map, float* npcs_map, float* fit_npcs, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_points_winner(const float* xyz, const int64_t* scene_offsets, int64_t n_total, const double* trans, int S, int H, int W,
                      double fx, double fy, double u0, double v0, int32_t* winner, gpn_stream_t stream);
int gpn_points_paint(const int32_t* winner, const int64_t* scene_offsets, int S, int H, int W, const gpn_visu_layer_t* layers_host,
                     int n_layers, const uint8_t* palette, int K, int edge, int CH, int CW, uint8_t* canvas, gpn_stream_t stream);
size_t gpn_boxes_draw_ws_bytes(int S, int H, int W);
int gpn_boxes_draw(const double* bbox, const int32_t* box_scene, int64_t Q, const double* trans, int S, int H, int W, double fx,
                   double fy, double u0, double v0, const int32_t* tiles_host, int n_tiles, int edge, int CH, int CW,
                   uint8_t* canvas, void* ws, size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * GR - class labels for class-agnostic 2D masks ("grounding"): everything between "pixel masks + an image feature map" and "the
 * part class of every mask".  Reference: structure/utils.py:491-497 (mask_change_reso), structure/gapartnet.py:145-158
 * (mask_fea_process / sam_mask_fea_process), utils.py:499-528 (load_data_single_file, KNN_classifier), gapartnet.py:180-204
 * (get_GAPart_grounding_result / get_sam_grounding_result).  The feature extractor and the segmenter are the caller's.  No float
 * atomics, every reduction has a fixed shape, nothing is read back; a mask's or a query's result is bit-equal whatever else is in
 * the call.  Counts of 0 (K, Q) are valid calls that launch nothing.
 * gpn_ground_mask_resize: binary masks [K,H,W] u8 (non-zero = member) -> levels [K,Hf,Wf] u8 in 0..128 (0 = fully inside).  For a
 *   0/1 mask the reference's detour (colour map -> PIL.Image.resize -> first channel -> clip(0,128)) is Pillow's default (bicubic)
 *   resize of the 8-bit image 128 (1 - m), clipped to 0..128, and this is that resize byte for byte: a horizontal pass to a u8
 *   intermediate [K,H,Wf] (the workspace), then a vertical pass, each out = clip8((2^21 + sum_j coef[j] * in[first + j]) >> 22) in
 *   32-bit integers.  The coefficient tables are Pillow's (bicubic a = -0.5, support 2 max(1, in/out), normalised in double,
 *   trunc(+-0.5 + w 2^22)); the caller computes them on the host: xbounds_host [Wf,2] i32 = (first, count), xcoef_host
 *   [Wf,ksize_x] i32, the same for y, and tables_dev = the four arrays back to back on the device (xbounds | xcoef | ybounds |
 *   ycoef).  The host copies are only checked (0 <= first, count <= ksize, first + count <= the input extent: GPN_ERR_ARG before
 *   any launch), the kernels read tables_dev.  H, W, Hf, Wf <= GPN_GROUND_MAX_SIDE.  An equal size is the identity table, not a
 *   special case.  Float-valued masks are not supported.
 * gpn_ground_mask_pool: fea [V,Hf,Wf,C] f32, levels [K,Hf,Wf] u8, mask_view [K] i32 in 0..V-1 (clamped into it) -> feat [K,C] f32,
 *   feat[k,c] = max over (h,w) of fea[mask_view[k],h,w,c] * ((128 - min(level,128)) / 128).  The weight is a multiple of 1/128, so
 *   the one fp32 product is the only rounding.  A NaN product makes the result NaN (numpy's max); the sign of a zero result is
 *   unspecified.  A map is read once per group of 8 consecutive masks that share its view.
 * gpn_ground_bank_norms: bank [M,D] f32 -> norms [M] f32 = sum of squares (an fmaf chain per lane of a wave, then a shuffle tree).
 *   Once per bank.
 * gpn_ground_knn: queries [Q,D] f32, bank [M,D] f32, bank_norms [M], bank_labels [M] i32 -> nn_index [Q,k] i32 (ascending by
 *   distance), nn_d2 [Q,k] f32, votes [Q,n_classes] i32, label [Q] i32: KNeighborsClassifier(n_neighbors = k, brute force,
 *   uniform weights).kneighbors / .predict.  d2 = max(0, (|q|^2 + |b|^2) - 2 q.b) in fp32, the dot product an fmaf chain in a fixed
 *   order on the fp32 MFMA: |d2 - true| <= (D + 3) 2^-24 (|q|^2 + |b|^2).  Order: (d2, bank row) ascending - equal distances put the
 *   lower row first; equal votes give the smallest class id.  A NaN distance never becomes a neighbour; if fewer than k rows have
 *   a comparable distance the tail is index -1, d2 = +inf, no vote.  1 <= k <= GPN_GROUND_MAX_K, k <= M, D >= 1, 1 <= n_classes <=
 *   GPN_GROUND_MAX_CLASSES, else GPN_ERR_ARG before any launch.  bank_labels lives on the device and is not read by the host: a
 *   label outside 0..n_classes-1 casts no vote here, and the Python wrapper (PartGrounder) refuses such a bank when it is built.
 *   The bank is streamed once per tile of 64 queries: workgroups own slices of bank rows and a running top-k per query, a second
 *   launch merges the slices (workspace: gpn_ground_knn_ws_bytes).
 * ================================================================================================ */
#define GPN_GROUND_MAX_K 32
#define GPN_GROUND_MAX_CLASSES 64
#define GPN_GROUND_MAX_SIDE 4096
size_t gpn_ground_mask_resize_ws_bytes(int K, int H, int Wf);
int gpn_ground_mask_resize(const uint8_t* masks, int K, int H, int W, int Hf, int Wf, const int32_t* xbounds_host,
                           const int32_t* xcoef_host, int ksize_x, const int32_t* ybounds_host, const int32_t* ycoef_host, int ksize_y,
                           const int32_t* tables_dev, uint8_t* levels, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_ground_mask_pool(const float* fea, const uint8_t* levels, const int32_t* mask_view, int V, int Hf, int Wf, int C, int K,
                         float* feat, gpn_stream_t stream);
int gpn_ground_bank_norms(const float* bank, int64_t M, int D, float* norms, gpn_stream_t stream);
size_t gpn_ground_knn_ws_bytes(int64_t Q, int64_t M, int k);
int gpn_ground_knn(const float* queries, int64_t Q, const float* bank, const float* bank_norms, const int32_t* bank_labels, int64_t M,
                   int D, int k, int n_classes, int32_t* nn_index, float* nn_d2, int32_t* votes, int32_t* label, void* ws,
                   size_t ws_bytes, gpn_stream_t stream);

/* ================================================================================================
 * DEV - entry points whose extents are DEVICE COUNTERS (round 4: the proposal stage of a training step without a host read;
 * reference glue: network/model.py:228-346, 348-462 - there every stage boundary is a device->host read of a size).
 * Convention of every *_dev entry point: an extent argument (N, P, M, V ...) is the BOUND its buffers are allocated for;
 * `<x>_dev` points at an int64 on the device holding the live value (written by an earlier launch on the stream, e.g.
 * gpn_proposals_build's counts) and `<x>_plan` is the host's estimate of it (<= 0: none) that only sizes the grid.  Kernels read
 * the counter and walk their work with a grid stride, so results never depend on the estimate; tables are laid out for the LIVE
 * count (see gpn_net_slot_t).  Each computes exactly what its exactly-sized twin computes on the first *<x>_dev rows.
 * ================================================================================================ */
int gpn_rulebook_subm3_dev(const int32_t* indices, int64_t N, const int64_t* n_dev, int64_t n_plan,
                           const int32_t* spatial_shape_host, int32_t* nbr, int32_t* pair_src, int32_t* pair_dst,
                           int32_t* tile_off, int64_t* num_pairs, void* ws, size_t ws_bytes, gpn_stream_t stream);
size_t gpn_rulebook_down_dev_ws_bytes(int64_t N, int64_t batch_size, const int32_t* spatial_shape_host);
int gpn_rulebook_down_dev(const int32_t* indices, int64_t N, const int64_t* n_dev, int64_t n_plan, int64_t batch_size,
                          const int64_t* batch_dev, int64_t batch_plan, const int32_t* spatial_shape_host, int32_t* out_indices,
                          int32_t* fine_to_coarse, int32_t* tap, int64_t* num_out, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_rulebook_down_lists_dev(const int32_t* fine_to_coarse, const int32_t* tap, int64_t N, const int64_t* n_dev, int64_t n_plan,
                                int64_t n_out, const int64_t* n_out_dev, int64_t n_out_plan, int32_t* fwd_nbr, int32_t* fwd_src,
                                int32_t* fwd_dst, int32_t* fwd_tile_off, int32_t* bwd_nbr, int32_t* bwd_src, int32_t* bwd_dst,
                                int32_t* bwd_tile_off, int64_t* num_pairs, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_rulebook_identity_dev(int64_t n, const int64_t* n_dev, int64_t n_plan, int32_t* rows, int32_t* tile_off, int32_t* nbr,
                              int64_t* num_pairs, gpn_stream_t stream);
int gpn_gather_rows_dev(const float* table, const int32_t* idx, int64_t n, const int64_t* n_dev, int64_t n_plan, int C, float* out,
                        gpn_stream_t stream);
int gpn_scatter_rows_csr_dev(const float* dout, const int32_t* order, const int32_t* starts, int64_t n_rows, const int64_t* n_dev,
                             int64_t n_plan, int C, float* dtable, gpn_stream_t stream);
int gpn_proposals_voxel_mean_dev(const float* feats, const int64_t* point_indices, const int32_t* point_order,
                                 const int32_t* voxel_point_start, int64_t V, const int64_t* v_dev, int64_t v_plan, int C, float* out,
                                 gpn_stream_t stream);
/* sem_labels [N] i64 / gt_npcs [N,3] f32 (either may be NULL) at the proposal points: the reference's sem_labels[rows],
 * gt_npcs[rows] (model.py:556-571) for the first *m_dev of M rows */
int gpn_proposals_targets_dev(const int64_t* sem_labels, const float* gt_npcs, const int64_t* point_indices, int64_t M,
                              const int64_t* m_dev, int64_t m_plan, int64_t* sem_out, float* npcs_out, gpn_stream_t stream);
int gpn_linear_fwd_dev(const float* x, const float* W, const float* b, int64_t N, const int64_t* n_dev, int64_t n_plan, int cin,
                       int cout, float* y, gpn_stream_t stream);
int gpn_linear_bwd_dev(const float* x, const float* W, const float* dy, int64_t N, const int64_t* n_dev, int64_t n_plan, int cin,
                       int cout, float* dx, float* dW, float* db, void* ws, size_t ws_bytes, gpn_stream_t stream);
int gpn_segmented_maxpool_fwd_dev(const float* values, const int32_t* begin, const int32_t* end, int64_t P, const int64_t* p_dev,
                                  int64_t p_plan, int C, float* pooled, int32_t* argmax, gpn_stream_t stream);
int gpn_segmented_maxpool_bwd_dev(const float* dpooled, const int32_t* argmax, int64_t P, const int64_t* p_dev, int64_t p_plan, int C,
                                  int64_t M, const int64_t* m_dev, int64_t m_plan, float* dvalues, gpn_stream_t stream);
int gpn_instance_iou_dev(const int32_t* proposal_offsets, const int32_t* instance_labels, const int32_t* batch_indices,
                         const int32_t* num_points_per_instance, int64_t P, const int64_t* p_dev, int64_t p_plan, int64_t B, int I,
                         float* ious, gpn_stream_t stream);
int gpn_score_loss_dev(const float* logits, int C1, const int64_t* cls_i64, const int32_t* cls_i32, const int32_t* offsets,
                       const float* ious, int I, int64_t P, const int64_t* p_dev, float fg_thresh, float bg_thresh, float* loss,
                       float* score_preds, float* d_logits, gpn_stream_t stream);
int gpn_npcs_loss_fwd_dev(const float* logits, int n_cls3, const float* gt_npcs, const int32_t* sem_preds, const int64_t* sem_labels,
                          const int32_t* proposal_offsets, int64_t P, const int64_t* p_dev, int64_t p_plan,
                          const int64_t* sym_of_class, const float* mats, const int32_t* type_first, const int32_t* type_count,
                          const int32_t* type_group, int n_types, float* loss, void* scratch, gpn_stream_t stream);
int gpn_npcs_loss_bwd_dev(const float* logits, int n_cls3, const float* gt_npcs, const int32_t* sem_preds, const int64_t* sem_labels,
                          const int64_t* proposal_indices, int64_t M, const int64_t* m_dev, int64_t m_plan, int64_t P,
                          const int64_t* sym_of_class, const float* mats, const int32_t* type_first, const int32_t* type_count,
                          const int32_t* type_group, int n_types, const void* scratch, const float* grad_loss, float* d_logits,
                          gpn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GPN_H */
