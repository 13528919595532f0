// Fused render chains: the reference's per-batch sequence of callables collapsed into one host call
// that enqueues the kernels back to back on one stream (no host sync, no allocation).
//   plain : rendering.py:27-51   (cal_geometry)
//   styled: rendering.py:118-178 (render_style)   -- see mlp_style.hip
#include <cstdlib>

#include "common.h"

#include "mlp_pack.h"
#include "mlp_style_mx.h"
#include "render_args.h"

namespace tgtc {
int launch_composite(const float* rgb, const float* sigma, const float* ts, int64_t R, int N, float* rgb_exp,
                     float* t_exp, float* weights, hipStream_t st);
int launch_sample_fine(const double* rays_o, const double* rays_d, const float* ts, const float* weights, int64_t R,
                       int N, int n_fine, double* pts_out, float* ts_out, hipStream_t st);
int launch_coarse_to_fine(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out, float* weights_out,
                          uint32_t* took_sort, hipStream_t st);
int launch_composite_live_colours(const float* rgb, const float* sigma, const float* ts, int64_t R, int N, float* rgb_exp,
                                  float* t_exp, float* weights, hipStream_t st);
int nerf_forward_rays_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                           int N, float* rgb, float* sigma, hipStream_t st);

int styled_forward_rays_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                             const float* ts, const float* z, int64_t R, int N, float* rgb, float* sigma,
                             hipStream_t st);

int styled_forward_rays_multi_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                   const float* ts, const float* z, int K, int64_t R, int N, float* rgb, float* sigma,
                                   hipStream_t st);

int styled_forward_rays_sparse_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const float* ts, const float* z, int K, int64_t R, int N, const uint32_t* live,
                                    const uint32_t* n_live, float* rgb, hipStream_t st);
int launch_compact_live(const float* w, int64_t M, float min_weight, uint32_t* live, uint32_t* scratch, uint32_t* live_count,
                        hipStream_t st);
int launch_count_live(const float* w, int64_t M, float min_weight, uint32_t* scratch, hipStream_t st);
int launch_live_stat(uint32_t* scratch, int64_t M, const uint32_t** stat, hipStream_t st);
int nerf_forward_list_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                           const uint32_t* live, const uint32_t* n_live, float* rgb, hipStream_t st);
int nerf_stash_fill_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         float* sigma, uint32_t* scratch, uint32_t* ovf, hipStream_t st);
int nerf_stash_heads_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, int64_t R, int N, uint32_t* scratch,
                          float* rgb, hipStream_t st);

int styled_restyle_live_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                             const float* z, int K, int64_t R, int N, const uint32_t* live, const float* ts_live, int64_t count,
                             float* rgb_live, hipStream_t st);
int style_fold_latents_impl(const tgtc_net* style, const float* z, int K, float* folded, hipStream_t st);
int styled_forward_list_folded_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                    const uint32_t* n_live, float* rgb, hipStream_t st);
int styled_restyle_live_folded_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                                    int64_t count, float* rgb_live, hipStream_t st);
int styled_trunk_plane_impl(const tgtc_net* nerf, const double* rays_o, const double* rays_d, int64_t R, int N,
                            const uint32_t* live, const float* ts_live, int64_t count, void* plane, hipStream_t st);
int styled_restyle_plane_impl(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                              const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                              int64_t count, const void* plane, float* rgb_live, hipStream_t st);
int styled_trunk_plane_mx_impl(const tgtc_net* nerf, const double* rays_o, const double* rays_d, int64_t R, int N,
                               const uint32_t* live, const float* ts_live, int64_t count, void* plane, hipStream_t st);
int trunk_plane_read_impl(bool fp16, const void* plane, int64_t count, float* hi, float* lo, hipStream_t st);
int launch_composite_live(const uint32_t* ray_start, const uint32_t* live, const float* w_live, const float* rgb_live, int64_t R,
                          int N, int K, int64_t count, float* rgb_exp, hipStream_t st);
int launch_geometry_pack(const uint32_t* live, const float* ts_f, const float* w_f, const float* t_fine, int64_t R, int N,
                         int64_t count, float min_weight, uint32_t* header, float* t_out, uint32_t* ray_start, uint32_t* live_out,
                         float* ts_live, float* w_live, hipStream_t st);

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RenderWorkspace {
    float *ts_c, *sigma_c, *rgb_c, *w_c, *ts_f, *sigma_f, *rgb_f;
    size_t total;
    RenderWorkspace(char* base, int64_t R, int nc, int nf) {
        const int nt = nc + nf;
        size_t off = 0;
        auto take = [&](size_t floats) {
            float* p = reinterpret_cast<float*>(base + off);
            off += align256(floats * sizeof(float));
            return p;
        };
        ts_c = take((size_t)R * nc);
        sigma_c = take((size_t)R * nc);
        rgb_c = take((size_t)R * nc * 3);
        w_c = take((size_t)R * nc);
        ts_f = take((size_t)R * nt);
        sigma_f = take((size_t)R * nt);
        rgb_f = take((size_t)R * nt * 3);
        total = off;
    }
};

// The planes the multi-latent stylised chain uses: RenderWorkspace's without the coarse colours, rgb_f [K,R,Nc+Nf,3].
struct MultiWorkspace {
    float *ts_c, *sigma_c, *w_c, *ts_f, *sigma_f, *rgb_f;
    size_t total;
    MultiWorkspace(char* base, int64_t R, int nc, int nf, int K) {
        const int nt = nc + nf;
        size_t off = 0;
        auto take = [&](size_t floats) {
            float* p = reinterpret_cast<float*>(base + off);
            off += align256(floats * sizeof(float));
            return p;
        };
        ts_c = take((size_t)R * nc);
        sigma_c = take((size_t)R * nc);
        w_c = take((size_t)R * nc);
        ts_f = take((size_t)R * nt);
        sigma_f = take((size_t)R * nt);
        rgb_f = take((size_t)K * R * nt * 3);
        total = off;
    }
};

// The culled stylised chain: MultiWorkspace's six planes, then the fine weights w_f [R,Nc+Nf], the list live [R*(Nc+Nf)]
// and the fixed scratch of the compaction (word 0: the live count; mlp_style_sparse.hip).
struct SparseWorkspace {
    MultiWorkspace m;
    float* w_f;
    uint32_t *live, *scratch;
    size_t total;
    SparseWorkspace(char* base, int64_t R, int nc, int nf, int K) : m(base, R, nc, nf, K) {
        const size_t plane = align256((size_t)R * (nc + nf) * sizeof(float));
        w_f = reinterpret_cast<float*>(base + m.total);
        live = reinterpret_cast<uint32_t*>(base + m.total + plane);
        scratch = reinterpret_cast<uint32_t*>(base + m.total + 2 * plane);
        total = m.total + 2 * plane + kSparseScratchBytes;
    }
};

// A geometry cache (tgtc_geometry_pack): a 256-byte header, then t_fine [R], ray_start [R+1], live / ts_live / w_live [count],
// every plane rounded up to 256 bytes.
struct GeometryCacheLayout {
    uint32_t *header, *ray_start, *live;
    float *t, *ts_live, *w_live;
    size_t total;
    GeometryCacheLayout(char* base, int64_t R, int64_t count) {
        size_t off = 0;
        auto take = [&](size_t bytes) {
            char* p = base + off;
            off += align256(bytes);
            return p;
        };
        header = reinterpret_cast<uint32_t*>(take(256));
        t = reinterpret_cast<float*>(take((size_t)R * 4));
        ray_start = reinterpret_cast<uint32_t*>(take(((size_t)R + 1) * 4));
        live = reinterpret_cast<uint32_t*>(take((size_t)count * 4));
        ts_live = reinterpret_cast<float*>(take((size_t)count * 4));
        w_live = reinterpret_cast<float*>(take((size_t)count * 4));
        total = off;
    }
};
}  // namespace tgtc

using namespace tgtc;

extern "C" size_t tgtc_render_workspace_bytes(int64_t R, int n_coarse, int n_fine) {
    if (R < 0 || n_coarse < 0 || n_fine < 0) return 0;
    return RenderWorkspace(nullptr, R, n_coarse, n_fine).total;
}

// Is there a ray kernel for this render?  prec_s < 0: the plain kernel (render_fused.hip); otherwise the stylised one
// (render_styled_fused.hip), built for fp16x3 in all three handles.  The tiling limits are those of the per-wave LDS strip.
static bool ray_kernel_built(int prec_c, int prec_f, int prec_s, int n_coarse, int n_fine, int want_coarse) {
    const bool precs = prec_s < 0 ? (prec_c == TGTC_PREC_FP16X3 && (prec_f == TGTC_PREC_FP16X3 || prec_f == TGTC_PREC_FP16_FP6)) ||
                                        (prec_c == TGTC_PREC_FP16 && prec_f == TGTC_PREC_FP16)
                                  : prec_c == TGTC_PREC_FP16X3 && prec_f == TGTC_PREC_FP16X3 && prec_s == TGTC_PREC_FP16X3;
    const int step = prec_c == TGTC_PREC_FP16 ? 32 : 16;   // tiles per pass x 16 samples
    return precs && !want_coarse && n_fine >= 1 && n_coarse >= 16 && n_coarse % step == 0 && (n_coarse + n_fine) % step == 0 &&
           n_coarse <= kFusedMaxCoarse && n_coarse + n_fine <= kFusedMaxTotal;
}

extern "C" int tgtc_render_path(int request, int prec_coarse, int prec_fine, int prec_style, int n_coarse, int n_fine,
                                int want_coarse) {
    auto prec_ok = [](int p) { return p == TGTC_PREC_FP16X3 || p == TGTC_PREC_FP16 || p == TGTC_PREC_FP16_FP6; };
    TGTC_REQUIRE(request == TGTC_PATH_AUTO || request == TGTC_PATH_RAY_KERNEL || request == TGTC_PATH_CHAIN,
                 "render_path: bad request %d", request);
    TGTC_REQUIRE(prec_ok(prec_coarse) && prec_ok(prec_fine) && (prec_style == -1 || prec_ok(prec_style)),
                 "render_path: bad precision %d / %d / %d", prec_coarse, prec_fine, prec_style);
    // the reference dereferences None when N_samples_fine == 0; require it instead
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    const bool built = ray_kernel_built(prec_coarse, prec_fine, prec_style, n_coarse, n_fine, want_coarse);
    if (request == TGTC_PATH_RAY_KERNEL && !built)
        return fail(TGTC_ERR_UNSUPPORTED, "render: no ray kernel for precisions %d + %d (style %d), %d + %d samples%s",
                    prec_coarse, prec_fine, prec_style, n_coarse, n_fine, want_coarse ? ", coarse image" : "");
    // fp16x3 + fp16_fp6: the fine pass is faster on the two-tile per-sample kernel (mlp_nerf_mx2.hip: half the LDS bytes per
    // MFMA of any one-tile loop, the ray kernel's included) than inside the ray kernel, and the per-sample tensors it
    // needs are 0.3 % of the frame time in HBM traffic: AUTO takes the chain (the split path)
    const bool split = prec_coarse == TGTC_PREC_FP16X3 && prec_fine == TGTC_PREC_FP16_FP6;
    if (request == TGTC_PATH_AUTO) return built && !split ? TGTC_PATH_RAY_KERNEL : TGTC_PATH_CHAIN;
    return request;
}

// The depths-only instance of the plain ray kernel as an entry of its own: what the stylised chain, the multi-latent, the
// culled and the restyle renders launch internally, and what lets a test hold a ray kernel's pixel against a reference
// evaluated at the kernel's own fine depths (tests/test_ray_kernel_shapes_gpu.py).
extern "C" int tgtc_render_depths(const tgtc_net* coarse, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                                  int n_fine, float near_, float far_, const float* jitter, float* ts_out, void* stream) {
    TGTC_REQUIRE(coarse && R >= 0, "render_depths: bad argument");
    TGTC_REQUIRE(coarse->kind == 0, "render_depths: coarse must be a NeRF handle");
    if (coarse->precision == TGTC_PREC_FP16_FP6 ||
        !ray_kernel_built(coarse->precision, coarse->precision, -1, n_coarse, n_fine, 0))
        return fail(TGTC_ERR_UNSUPPORTED, "render_depths: no depths-only ray kernel for coarse precision %d, %d + %d samples",
                    coarse->precision, n_coarse, n_fine);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts_out, "render_depths: null pointer");
    FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, coarse->dev, nullptr, nullptr, ts_out};
    return launch_fused_depths(coarse->precision, a, as_stream(stream));
}

// ---- the per-ray stage between the passes: coarse densities -> weights -> fine depths
// A render that wants no coarse image needs the coarse weights for the inverse CDF alone: ONE kernel computes them, samples
// and merges (raypath.hip, coarse_to_fine_kernel), and the plane w_c stays unwritten.  With a coarse image asked, or with
// TGTC_PER_RAY_PAIR=1 in the environment (read at every render: the yardstick the one kernel is held against), the
// compositor writes w_c and the sampler reads it back.  The depths are the same bits either way.
static int coarse_to_fine(const float* rgb_c, const float* sigma_c, const float* ts_c, float* w_c, const double* rays_o,
                          const double* rays_d, int64_t R, int n_coarse, int n_fine, float* rgb_coarse, float* t_coarse,
                          float* ts_f, hipStream_t st) {
    if (!rgb_coarse && !t_coarse) {
        const char* e = std::getenv("TGTC_PER_RAY_PAIR");
        if (!(e && e[0] == '1')) return launch_coarse_to_fine(sigma_c, ts_c, R, n_coarse, n_fine, ts_f, nullptr, nullptr, st);
    }
    const int rc = launch_composite(rgb_c, sigma_c, ts_c, R, n_coarse, rgb_coarse, t_coarse, w_c, st);
    if (rc) return rc;
    return launch_sample_fine(rays_o, rays_d, ts_c, w_c, R, n_coarse, n_fine, nullptr, ts_f, st);
}

// ---- the two-phase fine pass of the plain chain
// A fine sample with sigma <= 0 has alpha = 1 - exp(-relu(sigma) delta) = 0 exactly, weight 0 x T = +0, and enters the pixel
// as acc + 0 x c: for finite colours the image does not need its colour head.  With the live share L of the samples, f the
// full fine launch and s the density-only one, "densities, compaction, colours of the listed samples, a compositor that
// reads colours at live samples only" costs s + L f + ~0.5 ms against f, a gain while L < L* = 1 - s / f.
// kCullLiveThreshold = L* less a margin, both measured on the MI355X (tools/time_plain_cull.py --step0,
// profiles/plain_cull_timing.json): on the fine depths of a real 400 x 400 render at 128 + 64, f = 53.10 ms and
// s = 43.75 ms, L* = 0.176.  The margin is the whole spread of the live
// share over the benchmark's orbit (spiral_pose 0 .. 119: 0.098 .. 0.127, so 0.029; consecutive poses differ by 0.0013 at
// most), which lets the statistic come from ANY frame of the orbit, plus the fixed cost of the extra launches (0.4 ms of
// f, 0.007): 0.176 - 0.029 - 0.007 = 0.14.
constexpr float kCullLiveThreshold = 0.14f;

// AUTO: cull iff the last share that LANDED in the handle's pinned word is below the threshold; nothing landed yet, or a
// word that cannot be a (live, total) pair: dense.  The read never waits for the device, and both branches give the same
// bits, so what a caller cannot know -- whether its previous render has finished -- only ever changes the time.
static bool cull_wanted(const tgtc_cull_state* c) {
    if (c->mode != TGTC_CULL_AUTO) return c->mode == TGTC_CULL_ON;
    const uint64_t word = *c->landed;
    const uint32_t live = (uint32_t)word, total = (uint32_t)(word >> 32);
    return total != 0 && live <= total && (double)live < (double)kCullLiveThreshold * (double)total;
}

// The fine pass and the fine image of the plain chain.  The list and the compaction's scratch live in the planes that are
// dead once the fine depths exist (ts_c, sigma_c, rgb_c, w_c: contiguous, and the coarse image has been composited): the
// workspace does not grow.  Where they do not fit, or the samples cannot be indexed by 32 bits, the pass is dense.
static int fine_pass(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int nt,
                     const RenderWorkspace& ws, float* rgb_fine, float* t_fine, hipStream_t st) {
    const int64_t M = R * (int64_t)nt;
    char* const dead = reinterpret_cast<char*>(ws.ts_c);
    const size_t dead_bytes = (size_t)(reinterpret_cast<char*>(ws.ts_f) - dead);
    tgtc_cull_state* const c = fine->cull;
    const bool listable = c && fine->precision == TGTC_PREC_FP16_FP6 && M < ((int64_t)1 << 31);
    const bool cull = listable && dead_bytes >= (size_t)M * 4 + kSparseScratchBytes && cull_wanted(c);
    uint32_t* scratch = nullptr;
    int rc;
    if (cull && fine->stash) {
        // the stashed form (mlp_nerf_mx2_stash.hip): the density launch parks layer 7's output of its live samples, the
        // heads-only launch reads it back; live samples that found their wave's region full are the list of the list launch
        // (which runs its prologue alone when there are none).  The per-wave counts are the statistic's parts.
        uint32_t* const ovf = reinterpret_cast<uint32_t*>(dead);
        scratch = reinterpret_cast<uint32_t*>(dead + (size_t)M * 4);
        rc = nerf_stash_fill_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ws.sigma_f, scratch, ovf, st);
        if (rc) return rc;
        rc = nerf_stash_heads_impl(fine, rays_o, rays_d, R, nt, scratch, ws.rgb_f, st);
        if (rc) return rc;
        rc = nerf_forward_list_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ovf, scratch, ws.rgb_f, st);
        if (rc) return rc;
        ++c->culled;
    } else if (cull) {
        uint32_t* const live = reinterpret_cast<uint32_t*>(dead);
        scratch = reinterpret_cast<uint32_t*>(dead + (size_t)M * 4);
        rc = nerf_forward_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, nullptr, ws.sigma_f, st);
        if (rc) return rc;
        rc = launch_compact_live(ws.sigma_f, M, 0.0f, live, scratch, nullptr, st);
        if (rc) return rc;
        rc = nerf_forward_list_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, live, scratch, ws.rgb_f, st);
        if (rc) return rc;
        ++c->culled;
    } else {
        rc = nerf_forward_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ws.rgb_f, ws.sigma_f, st);
        if (rc) return rc;
        // the statistic alone: one run of the compaction's count kernel over sigma_f
        if (listable && c->mode != TGTC_CULL_OFF && dead_bytes >= kSparseScratchBytes) {
            scratch = reinterpret_cast<uint32_t*>(dead);
            rc = launch_count_live(ws.sigma_f, M, 0.0f, scratch, st);
            if (rc) return rc;
        }
        if (c) ++c->dense;
    }
    // culled: rgb_f holds colours at the listed samples (sigma > 0) and whatever the plane held before everywhere else; the
    // compositor reads it at the samples with sigma > 0 alone -- the bits of the plain instance over a zero-filled plane
    rc = cull ? launch_composite_live_colours(ws.rgb_f, ws.sigma_f, ws.ts_f, R, nt, rgb_fine, t_fine, nullptr, st)
              : launch_composite(ws.rgb_f, ws.sigma_f, ws.ts_f, R, nt, rgb_fine, t_fine, nullptr, st);
    if (rc) return rc;
    if (scratch) {
        // (live count, M) -> the handle's pinned word, asynchronously; the next render's AUTO reads whatever has landed
        const uint32_t* stat = nullptr;
        rc = launch_live_stat(scratch, M, &stat, st);
        if (rc) return rc;
        TGTC_HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t*>(c->landed), stat, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    return TGTC_OK;
}

// The plain render: ONE launch of the fused ray kernel (render_fused.hip; the workspace is not touched) or the chain of
// per-sample kernels through the workspace, as `path` resolves.
extern "C" int tgtc_render_rays_plain(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o,
                                      const double* rays_d, int64_t R, int n_coarse, int n_fine, float near_,
                                      float far_, const float* jitter, int path, void* workspace, size_t workspace_bytes,
                                      float* rgb_fine, float* t_fine, float* rgb_coarse, float* t_coarse,
                                      void* stream) {
    TGTC_REQUIRE(coarse && fine && R >= 0, "render_rays_plain: bad argument");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0, "render_rays_plain: coarse and fine must be NeRF handles");
    path = tgtc_render_path(path, coarse->precision, fine->precision, -1, n_coarse, n_fine, rgb_coarse || t_coarse);
    if (path < 0) return path;
    if (R == 0) return TGTC_OK;
    if (path == TGTC_PATH_RAY_KERNEL) {
        TGTC_REQUIRE(rays_o && rays_d && rgb_fine && t_fine, "render_rays_plain: null pointer");
        FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, fine->dev, rgb_fine, t_fine, nullptr};
        return launch_fused_render(coarse->precision, fine->precision, a, as_stream(stream));
    }
    TGTC_REQUIRE(rays_o && rays_d && workspace && rgb_fine && t_fine, "render_rays_plain: null pointer");
    RenderWorkspace ws(static_cast<char*>(workspace), R, n_coarse, n_fine);
    TGTC_REQUIRE(workspace_bytes >= ws.total, "render_rays_plain: workspace of %zu bytes, need %zu", workspace_bytes,
                 ws.total);
    hipStream_t st = as_stream(stream);
    int rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
    if (rc) return rc;
    // coarse pass: only the weights are consumed unless the caller asks for the coarse image
    float* rgb_c = rgb_coarse ? ws.rgb_c : nullptr;
    rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, rgb_c, ws.sigma_c, st);
    if (rc) return rc;
    rc = coarse_to_fine(rgb_c, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, rgb_coarse, t_coarse, ws.ts_f, st);
    if (rc) return rc;
    // fine pass + fine image: dense, or densities first and the colour head on the live samples only (fine_pass above)
    return fine_pass(fine, rays_o, rays_d, R, n_coarse + n_fine, ws, rgb_fine, t_fine, st);
}

// rendering.py:118-178 (render_style): ONE launch of the stylised ray kernel (render_styled_fused.hip; the workspace is not
// touched) or the stylised chain of per-sample kernels through the workspace, as `path` resolves.  The chain is the plain
// one with the stylised colour on both passes.  The coarse colours only matter if the caller asks for the coarse image: the
// fine sampler consumes the weights, which depend on sigma alone, so by default the coarse pass runs the sigma-only NeRF
// kernel -- or, where the plain ray kernel is built for the coarse precision, its first half (coarse depths -> coarse sigma
// -> weights -> fine depths, which then never leave the ray kernel).
extern "C" int tgtc_render_rays_styled(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                       const double* rays_o, const double* rays_d, const float* z, int64_t R,
                                       int n_coarse, int n_fine, float near_, float far_, const float* jitter, int path,
                                       void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                       float* rgb_coarse, float* t_coarse, void* stream) {
    TGTC_REQUIRE(coarse && fine && style && R >= 0, "render_rays_styled: bad argument");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "render_rays_styled: coarse and fine must be NeRF handles, style a style handle");
    const int want_coarse = rgb_coarse || t_coarse;
    path = tgtc_render_path(path, coarse->precision, fine->precision, style->precision, n_coarse, n_fine, want_coarse);
    if (path < 0) return path;
    if (R == 0) return TGTC_OK;
    if (path == TGTC_PATH_RAY_KERNEL) {
        TGTC_REQUIRE(rays_o && rays_d && z && rgb_fine && t_fine, "render_rays_styled: null pointer");
        FusedStyledArgs a{};
        a.ray = FusedArgs{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, fine->dev, rgb_fine, t_fine, nullptr};
        a.z = z, a.pair_bias = style->dev, a.concat_stream = style->dev + style->bias_bytes;
        a.style_stream = style->dev + style->stream2_off, a.slab = style->dev + style->stash_off;
        return launch_fused_styled(coarse->precision, a, style->n_wg, as_stream(stream));
    }
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled: null pointer");
    RenderWorkspace ws(static_cast<char*>(workspace), R, n_coarse, n_fine);
    TGTC_REQUIRE(workspace_bytes >= ws.total, "render_rays_styled: workspace of %zu bytes, need %zu", workspace_bytes,
                 ws.total);
    hipStream_t st = as_stream(stream);
    int rc;
    if (ray_kernel_built(coarse->precision, coarse->precision, -1, n_coarse, n_fine, want_coarse)) {
        FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, coarse->dev, nullptr, nullptr, ws.ts_f};
        rc = launch_fused_depths(coarse->precision, a, st);
        if (rc) return rc;
        rc = styled_forward_rays_impl(fine, style, rays_o, rays_d, ws.ts_f, z, R, n_coarse + n_fine, ws.rgb_f, ws.sigma_f, st);
        if (rc) return rc;
        return launch_composite(ws.rgb_f, ws.sigma_f, ws.ts_f, R, n_coarse + n_fine, rgb_fine, t_fine, nullptr, st);
    }
    rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
    if (rc) return rc;
    float* rgb_c = rgb_coarse ? ws.rgb_c : nullptr;
    if (rgb_c)
        rc = styled_forward_rays_impl(coarse, style, rays_o, rays_d, ws.ts_c, z, R, n_coarse, rgb_c, ws.sigma_c, st);
    else
        rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, nullptr, ws.sigma_c, st);
    if (rc) return rc;
    rc = coarse_to_fine(rgb_c, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, rgb_coarse, t_coarse, ws.ts_f, st);
    if (rc) return rc;
    rc = styled_forward_rays_impl(fine, style, rays_o, rays_d, ws.ts_f, z, R, n_coarse + n_fine, ws.rgb_f, ws.sigma_f, st);
    if (rc) return rc;
    return launch_composite(ws.rgb_f, ws.sigma_f, ws.ts_f, R, n_coarse + n_fine, rgb_fine, t_fine, nullptr, st);
}

extern "C" size_t tgtc_render_styled_multi_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K) {
    if (R < 0 || n_coarse < 0 || n_fine < 0 || K < 1) return 0;
    return MultiWorkspace(nullptr, R, n_coarse, n_fine, K).total;
}

// The stylised render under K latent sets per ray: the geometry half of the stylised chain above (coarse depths -> sigma ->
// weights -> fine depths) once, ONE launch of styled_rays_multi_kernel (mlp_style_multi.hip: the fine NeRF trunk once per
// sample, the concat and style MLPs once per sample and latent), then each rgb[k] composited with the shared sigma_f / ts_f.
extern "C" int tgtc_render_rays_styled_multi(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                             const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                             int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                             void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                             void* stream) {
    TGTC_REQUIRE(coarse && fine && style && R >= 0, "render_rays_styled_multi: bad argument");
    TGTC_REQUIRE(K >= 1, "render_rays_styled_multi: need K >= 1 latent sets (got %d)", K);
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "render_rays_styled_multi: coarse and fine must be NeRF handles, style a style handle");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    TGTC_REQUIRE(fine->precision == style->precision,
                 "render_rays_styled_multi: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled_multi: null pointer");
    const int nt = n_coarse + n_fine;
    if (R >= ((int64_t)1 << 31) || R * nt >= ((int64_t)1 << 31) || R * nt * K >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "render_rays_styled_multi: K x R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    MultiWorkspace ws(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    TGTC_REQUIRE(workspace_bytes >= ws.total, "render_rays_styled_multi: workspace of %zu bytes, need %zu", workspace_bytes,
                 ws.total);
    hipStream_t st = as_stream(stream);
    int rc;
    if (ray_kernel_built(coarse->precision, coarse->precision, -1, n_coarse, n_fine, 0)) {
        FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, coarse->dev, nullptr, nullptr, ws.ts_f};
        rc = launch_fused_depths(coarse->precision, a, st);
        if (rc) return rc;
    } else {
        rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
        if (rc) return rc;
        rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, nullptr, ws.sigma_c, st);
        if (rc) return rc;
        rc = coarse_to_fine(nullptr, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, nullptr, nullptr, ws.ts_f, st);
        if (rc) return rc;
    }
    rc = styled_forward_rays_multi_impl(fine, style, rays_o, rays_d, ws.ts_f, z, K, R, nt, ws.rgb_f, ws.sigma_f, st);
    if (rc) return rc;
    for (int k = 0; k < K; ++k) {
        rc = launch_composite(ws.rgb_f + (size_t)k * R * nt * 3, ws.sigma_f, ws.ts_f, R, nt, rgb_fine + (size_t)k * R * 3, t_fine,
                              nullptr, st);
        if (rc) return rc;
    }
    return TGTC_OK;
}

extern "C" size_t tgtc_render_styled_sparse_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K) {
    if (R < 0 || n_coarse < 0 || n_fine < 0 || K < 1) return 0;
    return SparseWorkspace(nullptr, R, n_coarse, n_fine, K).total;
}

// Steps 1-4 of the culled stylised render, the half that depends on the ray alone (tgtc_render_rays_styled_sparse and
// tgtc_geometry_build): fine depths ts_f, sigma_f, the depth image, the weights plane w_f, the ascending list live[] of the
// samples with w_f > min_weight and its length (scratch word 0, and *live_count where given).
static int ray_geometry(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R,
                        int n_coarse, int n_fine, float near_, float far_, const float* jitter, float min_weight,
                        const SparseWorkspace& sw, float* t_fine, uint32_t* live_count, void* stream) {
    const MultiWorkspace& ws = sw.m;
    const int nt = n_coarse + n_fine;
    hipStream_t st = as_stream(stream);
    int rc;
    // 1. geometry half, as tgtc_render_rays_styled_multi
    if (ray_kernel_built(coarse->precision, coarse->precision, -1, n_coarse, n_fine, 0)) {
        FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, coarse->dev, nullptr, nullptr, ws.ts_f};
        rc = launch_fused_depths(coarse->precision, a, st);
        if (rc) return rc;
    } else {
        rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
        if (rc) return rc;
        rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, nullptr, ws.sigma_c, st);
        if (rc) return rc;
        rc = coarse_to_fine(nullptr, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, nullptr, nullptr, ws.ts_f, st);
        if (rc) return rc;
    }
    // 2. sigma of every fine sample (the sigma-only NeRF launch carries the bits of the styled kernels' sigma:
    //    tests/test_sparse_style_gpu.py, test_sigma_pass_bits_of_the_styled_kernel)
    rc = nerf_forward_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, nullptr, ws.sigma_f, st);
    if (rc) return rc;
    // 3. depth image and the weights plane
    rc = launch_composite(nullptr, ws.sigma_f, ws.ts_f, R, nt, nullptr, t_fine, sw.w_f, st);
    if (rc) return rc;
    // 4. the ascending list of samples with w > min_weight
    return launch_compact_live(sw.w_f, R * (int64_t)nt, min_weight, sw.live, sw.scratch, live_count, st);
}

// The multi-latent stylised render with the style networks only on the samples whose compositing weight exceeds
// min_weight: geometry half as above, a sigma-only pass of the fine NeRF over every sample, the existing compositing kernel
// for depth + weights, the compaction, then the indexed multi-latent kernel (mlp_style_sparse.hip) into zero-filled colour
// planes and K compositing launches over the shared sigma / depths.
extern "C" int tgtc_render_rays_styled_sparse(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                              const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                              int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                              float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                              float* t_fine, uint32_t* live_count, void* stream) {
    TGTC_REQUIRE(K >= 1, "render_rays_styled_sparse: need K >= 1 latent sets (got %d)", K);
    TGTC_REQUIRE(min_weight >= 0.0f, "render_rays_styled_sparse: min_weight must be >= 0 and not NaN (got %g)", (double)min_weight);
    TGTC_REQUIRE(coarse && fine && style && R >= 0, "render_rays_styled_sparse: bad argument");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "render_rays_styled_sparse: coarse and fine must be NeRF handles, style a style handle");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    TGTC_REQUIRE(fine->precision == style->precision,
                 "render_rays_styled_sparse: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled_sparse: null pointer");
    const int nt = n_coarse + n_fine;
    if (R >= ((int64_t)1 << 31) || R * nt >= ((int64_t)1 << 31) || R * nt * K >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "render_rays_styled_sparse: K x R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    TGTC_REQUIRE(workspace_bytes >= sw.total, "render_rays_styled_sparse: workspace of %zu bytes, need %zu", workspace_bytes,
                 sw.total);
    const MultiWorkspace& ws = sw.m;
    hipStream_t st = as_stream(stream);
    // 1-4. everything that depends on the ray alone
    int rc = ray_geometry(coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, t_fine,
                          live_count, stream);
    if (rc) return rc;
    // 5. dead samples keep colour +0
    TGTC_HIP_CHECK(hipMemsetAsync(ws.rgb_f, 0, (size_t)K * R * nt * 3 * sizeof(float), st));
    // 6. trunk + concat MLP + style MLP over the list
    rc = styled_forward_rays_sparse_impl(fine, style, rays_o, rays_d, ws.ts_f, z, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    if (rc) return rc;
    // 7. compositing over the shared sigma / depths
    for (int k = 0; k < K; ++k) {
        rc = launch_composite(ws.rgb_f + (size_t)k * R * nt * 3, ws.sigma_f, ws.ts_f, R, nt, rgb_fine + (size_t)k * R * 3, nullptr,
                              nullptr, st);
        if (rc) return rc;
    }
    return TGTC_OK;
}

// ------------------------------------------------------------------------------------------------ geometry cache + restyle
// The ray-only half of the culled render kept as a compact device buffer, and "the same rays under new latents" from it:
// one launch of the compact indexed kernel over the cached list, one compositing launch over (latent, ray).

// Steps 1-4 of tgtc_render_rays_styled_sparse on the sparse workspace at K = 1.  The depth image also stays in the
// workspace (the first R floats of the colour plane, which no step of the build uses), where tgtc_geometry_pack reads it.
extern "C" int tgtc_geometry_build(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d,
                                   int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                   float min_weight, void* workspace, size_t workspace_bytes, float* t_fine,
                                   uint32_t* live_count, void* stream) {
    TGTC_REQUIRE(min_weight >= 0.0f, "geometry_build: min_weight must be >= 0 and not NaN (got %g)", (double)min_weight);
    TGTC_REQUIRE(coarse && fine && R >= 0, "geometry_build: bad argument");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0, "geometry_build: coarse and fine must be NeRF handles");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && workspace && live_count, "geometry_build: null pointer");
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_build: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, 1);
    TGTC_REQUIRE(workspace_bytes >= sw.total, "geometry_build: workspace of %zu bytes, need %zu", workspace_bytes, sw.total);
    int rc = ray_geometry(coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, sw.m.rgb_f,
                          live_count, stream);
    if (rc) return rc;
    if (t_fine)
        TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, sw.m.rgb_f, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return TGTC_OK;
}

extern "C" size_t tgtc_geometry_cache_bytes(int64_t R, int64_t count) {
    if (R < 0 || count < 0) return 0;
    return GeometryCacheLayout(nullptr, R, count).total;
}

extern "C" int tgtc_geometry_pack(const void* workspace, int64_t R, int n_coarse, int n_fine, float min_weight, int64_t count,
                                  void* cache, size_t cache_bytes, void* stream) {
    TGTC_REQUIRE(min_weight >= 0.0f, "geometry_pack: min_weight must be >= 0 and not NaN (got %g)", (double)min_weight);
    TGTC_REQUIRE(R >= 0 && count >= 0, "geometry_pack: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    TGTC_REQUIRE(workspace && cache, "geometry_pack: null pointer");
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_pack: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt, "geometry_pack: count %lld exceeds the %lld samples", (long long)count, (long long)(R * nt));
    GeometryCacheLayout gc(static_cast<char*>(cache), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "geometry_pack: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    SparseWorkspace sw(static_cast<char*>(const_cast<void*>(workspace)), R, n_coarse, n_fine, 1);
    return launch_geometry_pack(sw.live, sw.m.ts_f, sw.w_f, sw.m.rgb_f, R, nt, count, min_weight, gc.header, gc.t, gc.ray_start,
                                gc.live, gc.ts_live, gc.w_live, as_stream(stream));
}

extern "C" size_t tgtc_restyle_workspace_bytes(int64_t count, int K) {
    if (count < 0 || K < 1) return 0;
    return align256((size_t)K * (size_t)count * 3 * sizeof(float));
}

extern "C" int tgtc_restyle_rays(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                 const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                 size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                 float* t_fine, void* stream) {
    TGTC_REQUIRE(K >= 1, "restyle_rays: need K >= 1 latent sets (got %d)", K);
    TGTC_REQUIRE(fine && style && R >= 0 && count >= 0, "restyle_rays: bad argument");
    TGTC_REQUIRE(fine->kind == 0 && style->kind == 1, "restyle_rays: fine must be a NeRF handle, style a style handle");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    TGTC_REQUIRE(fine->precision == style->precision,
                 "restyle_rays: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && cache && rgb_fine && (workspace || count == 0), "restyle_rays: null pointer");
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt, "restyle_rays: count %lld exceeds the %lld samples", (long long)count, (long long)(R * nt));
    if (K * count >= ((int64_t)1 << 31) || K * R >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays: K x count >= 2^31 (fewer latents per call)");
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "restyle_rays: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    const size_t need = tgtc_restyle_workspace_bytes(count, K);
    TGTC_REQUIRE(workspace_bytes >= need, "restyle_rays: workspace of %zu bytes, need %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* rgb_live = static_cast<float*>(workspace);
    int rc;
    // 1. trunk + concat MLP + style MLP over the cached list into the compact colour planes (nothing to launch for an empty list)
    if (count > 0) {
        rc = styled_restyle_live_impl(fine, style, rays_o, rays_d, z, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        if (rc) return rc;
    }
    // 2. every (latent, ray): the colour sums of the dense compositing kernel; a ray without live samples gets +0
    rc = launch_composite_live(gc.ray_start, gc.live, gc.w_live, rgb_live, R, nt, K, count, rgb_fine, st);
    if (rc) return rc;
    // 3. the depth image
    if (t_fine) TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, gc.t, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TGTC_OK;
}

// ------------------------------------------------------------------------------------------------ frame-constant latents
// The culled render and the restyle for latents that do not depend on the ray: z [K,32].  The latent k-step of every layer
// of the two style networks is folded into K bias tables (tgtc_style_fold_latents, mlp_style.hip) kept in one more plane
// at the end of the workspace, and the folded instances of the indexed kernels (mlp_style_sparse.hip) run on the streams
// packed without that k-step.  Everything else is the unfolded sibling's.

extern "C" int tgtc_styled_forward_list_folded(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                               const double* rays_d, const float* ts, const void* folded, int K, int64_t R,
                                               int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    TGTC_REQUIRE(K >= 1, "styled_forward_list_folded: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(R >= 0 && N >= 1, "styled_forward_list_folded: bad argument");
    constexpr int64_t kLimit = (int64_t)1 << 31;
    if (R >= kLimit || R * (int64_t)N >= kLimit || R * (int64_t)N * K >= kLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "styled_forward_list_folded: K x R x N >= 2^31 in one launch (chunk the rays)");
    TGTC_REQUIRE(nerf && style, "styled_forward_list_folded: null handle");
    TGTC_REQUIRE(nerf->kind == 0 && style->kind == 1, "styled_forward_list_folded: nerf must be a NeRF handle, style a style handle");
    TGTC_REQUIRE(nerf->precision == style->precision,
                 "styled_forward_list_folded: NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && folded && live && n_live && rgb, "styled_forward_list_folded: null pointer");
    return styled_forward_list_folded_impl(nerf, style, rays_o, rays_d, ts, folded, K, R, N, live, n_live, rgb, as_stream(stream));
}

extern "C" size_t tgtc_render_styled_sparse_folded_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K) {
    if (R < 0 || n_coarse < 0 || n_fine < 0 || K < 1) return 0;
    return SparseWorkspace(nullptr, R, n_coarse, n_fine, K).total + align256(tgtc_style_folded_bytes(K));
}

extern "C" int tgtc_render_rays_styled_sparse_folded(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                                     const double* rays_o, const double* rays_d, const float* z, int K,
                                                     int64_t R, int n_coarse, int n_fine, float near_, float far_,
                                                     const float* jitter, float min_weight, void* workspace,
                                                     size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                                     uint32_t* live_count, void* stream) {
    TGTC_REQUIRE(K >= 1, "render_rays_styled_sparse_folded: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(min_weight >= 0.0f, "render_rays_styled_sparse_folded: min_weight must be >= 0 and not NaN (got %g)",
                 (double)min_weight);
    TGTC_REQUIRE(R >= 0, "render_rays_styled_sparse_folded: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R >= ((int64_t)1 << 31) || R * nt >= ((int64_t)1 << 31) || R * nt * K >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "render_rays_styled_sparse_folded: K x R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(coarse && fine && style, "render_rays_styled_sparse_folded: null handle");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "render_rays_styled_sparse_folded: coarse and fine must be NeRF handles, style a style handle");
    TGTC_REQUIRE(fine->precision == style->precision,
                 "render_rays_styled_sparse_folded: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled_sparse_folded: null pointer");
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    const size_t need = sw.total + align256(tgtc_style_folded_bytes(K));
    TGTC_REQUIRE(workspace_bytes >= need, "render_rays_styled_sparse_folded: workspace of %zu bytes, need %zu", workspace_bytes, need);
    float* folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + sw.total);
    const MultiWorkspace& ws = sw.m;
    hipStream_t st = as_stream(stream);
    // 0. the K bias tables
    int rc = style_fold_latents_impl(style, z, K, folded, st);
    if (rc) return rc;
    // 1-4. everything that depends on the ray alone
    rc = ray_geometry(coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, t_fine, live_count,
                      stream);
    if (rc) return rc;
    // 5. dead samples keep colour +0
    TGTC_HIP_CHECK(hipMemsetAsync(ws.rgb_f, 0, (size_t)K * R * nt * 3 * sizeof(float), st));
    // 6. trunk + folded concat MLP + folded style MLP over the list
    rc = styled_forward_list_folded_impl(fine, style, rays_o, rays_d, ws.ts_f, folded, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    if (rc) return rc;
    // 7. compositing over the shared sigma / depths
    for (int k = 0; k < K; ++k) {
        rc = launch_composite(ws.rgb_f + (size_t)k * R * nt * 3, ws.sigma_f, ws.ts_f, R, nt, rgb_fine + (size_t)k * R * 3, nullptr,
                              nullptr, st);
        if (rc) return rc;
    }
    return TGTC_OK;
}

extern "C" size_t tgtc_restyle_folded_workspace_bytes(int64_t count, int K) {
    if (count < 0 || K < 1) return 0;
    return tgtc_restyle_workspace_bytes(count, K) + align256(tgtc_style_folded_bytes(K));
}

extern "C" int tgtc_restyle_rays_folded(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                        const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                        size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes,
                                        float* rgb_fine, float* t_fine, void* stream) {
    TGTC_REQUIRE(K >= 1, "restyle_rays_folded: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(R >= 0 && count >= 0, "restyle_rays_folded: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays_folded: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt || R == 0, "restyle_rays_folded: count %lld exceeds the %lld samples", (long long)count,
                 (long long)(R * nt));
    if (K * count >= ((int64_t)1 << 31) || K * R >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays_folded: K x count >= 2^31 (fewer latents per call)");
    TGTC_REQUIRE(fine && style, "restyle_rays_folded: null handle");
    TGTC_REQUIRE(fine->kind == 0 && style->kind == 1, "restyle_rays_folded: fine must be a NeRF handle, style a style handle");
    TGTC_REQUIRE(fine->precision == style->precision,
                 "restyle_rays_folded: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && cache && rgb_fine && (workspace || count == 0), "restyle_rays_folded: null pointer");
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "restyle_rays_folded: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    const size_t need = tgtc_restyle_folded_workspace_bytes(count, K);
    TGTC_REQUIRE(workspace_bytes >= need, "restyle_rays_folded: workspace of %zu bytes, need %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* rgb_live = static_cast<float*>(workspace);
    float* folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + tgtc_restyle_workspace_bytes(count, K));
    int rc;
    // 1. the K bias tables, then trunk + folded concat MLP + folded style MLP over the cached list (nothing to launch for an
    //    empty list)
    if (count > 0) {
        rc = style_fold_latents_impl(style, z, K, folded, st);
        if (rc) return rc;
        rc = styled_restyle_live_folded_impl(fine, style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        if (rc) return rc;
    }
    // 2. every (latent, ray): the colour sums of the dense compositing kernel; a ray without live samples gets +0
    rc = launch_composite_live(gc.ray_start, gc.live, gc.w_live, rgb_live, R, nt, K, count, rgb_fine, st);
    if (rc) return rc;
    // 3. the depth image
    if (t_fine) TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, gc.t, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TGTC_OK;
}

// ------------------------------------------------------------------------------------------------ restyle from a trunk plane
// The last ray-only piece of a restyle -- the fine NeRF trunk, 556 800 of the 556 800 + K x 950 112 multiply-accumulates per
// live sample -- kept beside the cache: base_remap's operand fragments of every tile of the cached list in a caller-owned
// plane (tgtc_geometry_trunk), and the restyle from it, which runs the style networks alone and takes no NeRF handle.

extern "C" size_t tgtc_geometry_trunk_bytes(int precision, int64_t count) {
    if (count <= 0 || (precision != TGTC_PREC_FP16X3 && precision != TGTC_PREC_FP16)) return 0;
    const int64_t per_tile = precision == TGTC_PREC_FP16 ? 256 : 128;   // SAMPLES_PER_WG of the style kernels
    return (size_t)((count + per_tile - 1) / per_tile) * (size_t)131072;
}

extern "C" int tgtc_geometry_trunk(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                                   int n_fine, const void* cache, size_t cache_bytes, int64_t count, void* trunk,
                                   size_t trunk_bytes, void* stream) {
    TGTC_REQUIRE(R >= 0 && count >= 0, "geometry_trunk: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_trunk: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt || R == 0, "geometry_trunk: count %lld exceeds the %lld samples", (long long)count,
                 (long long)(R * nt));
    TGTC_REQUIRE(fine, "geometry_trunk: null handle");
    TGTC_REQUIRE(fine->kind == 0, "geometry_trunk: fine must be a NeRF handle");
    if (fine->precision != TGTC_PREC_FP16X3 && fine->precision != TGTC_PREC_FP16)
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_trunk: the style kernels are built for fp16x3 and fp16 handles only");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && cache && (trunk || count == 0), "geometry_trunk: null pointer");
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "geometry_trunk: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    const size_t need = tgtc_geometry_trunk_bytes(fine->precision, count);
    TGTC_REQUIRE(trunk_bytes >= need, "geometry_trunk: plane of %zu bytes, need %zu", trunk_bytes, need);
    if (count == 0) return TGTC_OK;
    return styled_trunk_plane_impl(fine, rays_o, rays_d, R, nt, gc.live, gc.ts_live, count, trunk, as_stream(stream));
}

// tgtc_restyle_rays / tgtc_restyle_rays_folded with the trunk read from the plane: the same workspaces, the same compositing
// launch and depth copy behind another style launch.
static int restyle_rays_trunk(const char* who, bool fold, bool mx, const tgtc_net* style, const double* rays_o, const double* rays_d,
                              const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes,
                              int64_t count, const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                              float* rgb_fine, float* t_fine, void* stream) {
    TGTC_REQUIRE(K >= 1, "%s: need K >= 1 latents (got %d)", who, K);
    TGTC_REQUIRE(R >= 0 && count >= 0, "%s: bad argument", who);
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31)) return fail(TGTC_ERR_UNSUPPORTED, "%s: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)", who);
    TGTC_REQUIRE(count <= R * nt || R == 0, "%s: count %lld exceeds the %lld samples", who, (long long)count, (long long)(R * nt));
    if (K * count >= ((int64_t)1 << 31) || K * R >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "%s: K x count >= 2^31 (fewer latents per call)", who);
    TGTC_REQUIRE(style, "%s: null handle", who);
    TGTC_REQUIRE(style->kind == 1, "%s: style must be a style handle", who);
    if (mx && !(style->mx && style->mx->dev))
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle has no fp16mx streams (tgtc_style_enable_mx)", who);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && cache && rgb_fine && (workspace || count == 0) && (trunk || count == 0),
                 "%s: null pointer", who);
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "%s: cache of %zu bytes, need %zu", who, cache_bytes, gc.total);
    const size_t need_plane = tgtc_geometry_trunk_bytes(style->precision, count);
    TGTC_REQUIRE(trunk_bytes >= need_plane, "%s: plane of %zu bytes, need %zu", who, trunk_bytes, need_plane);
    const size_t need = fold ? tgtc_restyle_folded_workspace_bytes(count, K) : tgtc_restyle_workspace_bytes(count, K);
    TGTC_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* rgb_live = static_cast<float*>(workspace);
    int rc;
    // 1. (the K bias tables, then) concat MLP + style MLP over the cached list, base_remap from the plane (nothing to launch
    //    for an empty list)
    if (count > 0) {
        float* folded = nullptr;
        if (fold) {
            folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + tgtc_restyle_workspace_bytes(count, K));
            rc = style_fold_latents_impl(style, z, K, folded, st);
            if (rc) return rc;
        }
        if (mx) rc = styled_restyle_plane_mx_impl(style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, trunk, rgb_live, st);
        else rc = styled_restyle_plane_impl(style, rays_o, rays_d, z, folded, K, R, nt, gc.live, gc.ts_live, count, trunk, rgb_live, st);
        if (rc) return rc;
    }
    // 2. every (latent, ray): the colour sums of the dense compositing kernel; a ray without live samples gets +0
    rc = launch_composite_live(gc.ray_start, gc.live, gc.w_live, rgb_live, R, nt, K, count, rgb_fine, st);
    if (rc) return rc;
    // 3. the depth image
    if (t_fine) TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, gc.t, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TGTC_OK;
}

extern "C" int tgtc_restyle_rays_trunk(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z, int K,
                                       int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                                       const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                                       float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays_trunk("restyle_rays_trunk", false, false, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache, cache_bytes,
                              count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

extern "C" int tgtc_restyle_rays_trunk_folded(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                                              int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes,
                                              int64_t count, const void* trunk, size_t trunk_bytes, void* workspace,
                                              size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays_trunk("restyle_rays_trunk_folded", true, false, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache,
                              cache_bytes, count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

// ... and with the style networks in fp16mx: the folded form on the handle's mx streams (tgtc_style_enable_mx; an fp16x3 handle,
// so the plane's size is checked as the fp16x3 plane's)
extern "C" int tgtc_restyle_rays_trunk_folded_mx(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                                                 int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                                 size_t cache_bytes, int64_t count, const void* trunk, size_t trunk_bytes,
                                                 void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                                 void* stream) {
    return restyle_rays_trunk("restyle_rays_trunk_folded_mx", true, true, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache,
                              cache_bytes, count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

// ------------------------------------------------------------------------------------------------ the plane from an fp16mx handle
// tgtc_geometry_trunk's arguments and checks in its order; the handle is in TGTC_PREC_FP16_FP6 and the plane it writes is the
// TGTC_PREC_FP16X3 plane (csrc/mlp_trunk_mx.hip)
extern "C" int tgtc_geometry_trunk_mx(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                                      int n_fine, const void* cache, size_t cache_bytes, int64_t count, void* trunk,
                                      size_t trunk_bytes, void* stream) {
    TGTC_REQUIRE(R >= 0 && count >= 0, "geometry_trunk_mx: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_trunk_mx: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt || R == 0, "geometry_trunk_mx: count %lld exceeds the %lld samples", (long long)count,
                 (long long)(R * nt));
    TGTC_REQUIRE(fine, "geometry_trunk_mx: null handle");
    TGTC_REQUIRE(fine->kind == 0, "geometry_trunk_mx: fine must be a NeRF handle");
    if (fine->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "geometry_trunk_mx: built for fp16mx handles only (tgtc_geometry_trunk takes fp16x3 and fp16)");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && cache && (trunk || count == 0), "geometry_trunk_mx: null pointer");
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "geometry_trunk_mx: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    const size_t need = tgtc_geometry_trunk_bytes(TGTC_PREC_FP16X3, count);
    TGTC_REQUIRE(trunk_bytes >= need, "geometry_trunk_mx: plane of %zu bytes, need %zu", trunk_bytes, need);
    if (count == 0) return TGTC_OK;
    return styled_trunk_plane_mx_impl(fine, rays_o, rays_d, R, nt, gc.live, gc.ts_live, count, trunk, as_stream(stream));
}

extern "C" int tgtc_geometry_trunk_read(int precision, const void* trunk, size_t trunk_bytes, int64_t count, float* hi, float* lo,
                                        void* stream) {
    TGTC_REQUIRE(count >= 0, "geometry_trunk_read: bad argument");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16X3 || precision == TGTC_PREC_FP16,
                 "geometry_trunk_read: a plane exists in fp16x3 and fp16 only (got precision %d)", precision);
    if (count >= ((int64_t)1 << 31)) return fail(TGTC_ERR_UNSUPPORTED, "geometry_trunk_read: count >= 2^31");
    if (count == 0) return TGTC_OK;
    TGTC_REQUIRE(trunk && hi, "geometry_trunk_read: null pointer");
    const size_t need = tgtc_geometry_trunk_bytes(precision, count);
    TGTC_REQUIRE(trunk_bytes >= need, "geometry_trunk_read: plane of %zu bytes, need %zu", trunk_bytes, need);
    return trunk_plane_read_impl(precision == TGTC_PREC_FP16, trunk, count, hi, lo, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------ the fp16x3+fp16mx pair, no plane
// The folded list entry points for a fine handle in TGTC_PREC_FP16_FP6 and an fp16x3 style handle with mx streams
// (csrc/mlp_list_mx.hip: trunk and latents of a tile in one persistent kernel, base_remap parked in slab region B of the style
// handle).  Arguments, workspaces, check order and the order of work are the siblings' (tgtc_styled_forward_list_folded,
// tgtc_render_rays_styled_sparse_folded, tgtc_restyle_rays_folded); only the rule for the handles' precisions differs.
static int list_mx_handles(const char* who, const tgtc_net* fine, const tgtc_net* style) {
    if (fine->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the NeRF handle must be in fp16mx (the siblings without _mx take fp16x3 and fp16)", who);
    if (style->precision != TGTC_PREC_FP16X3)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle must be in fp16x3 (an fp16 pair has no lo halves)", who);
    if (!(style->mx && style->mx->dev))
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle has no fp16mx streams (tgtc_style_enable_mx)", who);
    return TGTC_OK;
}

extern "C" int tgtc_styled_forward_list_folded_mx(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                                  const double* rays_d, const float* ts, const void* folded, int K, int64_t R,
                                                  int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    TGTC_REQUIRE(K >= 1, "styled_forward_list_folded_mx: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(R >= 0 && N >= 1, "styled_forward_list_folded_mx: bad argument");
    constexpr int64_t kLimit = (int64_t)1 << 31;
    if (R >= kLimit || R * (int64_t)N >= kLimit || R * (int64_t)N * K >= kLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "styled_forward_list_folded_mx: K x R x N >= 2^31 in one launch (chunk the rays)");
    TGTC_REQUIRE(nerf && style, "styled_forward_list_folded_mx: null handle");
    TGTC_REQUIRE(nerf->kind == 0 && style->kind == 1,
                 "styled_forward_list_folded_mx: nerf must be a NeRF handle, style a style handle");
    if (const int rc = list_mx_handles("styled_forward_list_folded_mx", nerf, style)) return rc;
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && folded && live && n_live && rgb, "styled_forward_list_folded_mx: null pointer");
    return styled_forward_list_folded_mx_impl(nerf, style, rays_o, rays_d, ts, folded, K, R, N, live, n_live, rgb, as_stream(stream));
}

extern "C" int tgtc_render_rays_styled_sparse_folded_mx(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                                        const double* rays_o, const double* rays_d, const float* z, int K,
                                                        int64_t R, int n_coarse, int n_fine, float near_, float far_,
                                                        const float* jitter, float min_weight, void* workspace,
                                                        size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                                        uint32_t* live_count, void* stream) {
    TGTC_REQUIRE(K >= 1, "render_rays_styled_sparse_folded_mx: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(min_weight >= 0.0f, "render_rays_styled_sparse_folded_mx: min_weight must be >= 0 and not NaN (got %g)",
                 (double)min_weight);
    TGTC_REQUIRE(R >= 0, "render_rays_styled_sparse_folded_mx: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R >= ((int64_t)1 << 31) || R * nt >= ((int64_t)1 << 31) || R * nt * K >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "render_rays_styled_sparse_folded_mx: K x R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(coarse && fine && style, "render_rays_styled_sparse_folded_mx: null handle");
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "render_rays_styled_sparse_folded_mx: coarse and fine must be NeRF handles, style a style handle");
    if (const int rc = list_mx_handles("render_rays_styled_sparse_folded_mx", fine, style)) return rc;
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled_sparse_folded_mx: null pointer");
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    const size_t need = sw.total + align256(tgtc_style_folded_bytes(K));
    TGTC_REQUIRE(workspace_bytes >= need, "render_rays_styled_sparse_folded_mx: workspace of %zu bytes, need %zu", workspace_bytes,
                 need);
    float* folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + sw.total);
    const MultiWorkspace& ws = sw.m;
    hipStream_t st = as_stream(stream);
    // 0. the K bias tables
    int rc = style_fold_latents_impl(style, z, K, folded, st);
    if (rc) return rc;
    // 1-4. everything that depends on the ray alone
    rc = ray_geometry(coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, t_fine, live_count,
                      stream);
    if (rc) return rc;
    // 5. dead samples keep colour +0
    TGTC_HIP_CHECK(hipMemsetAsync(ws.rgb_f, 0, (size_t)K * R * nt * 3 * sizeof(float), st));
    // 6. fp16mx trunk + the folded style pair's fp16mx streams over the list (the host never learns its length)
    rc = styled_forward_list_folded_mx_impl(fine, style, rays_o, rays_d, ws.ts_f, folded, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    if (rc) return rc;
    // 7. compositing over the shared sigma / depths
    for (int k = 0; k < K; ++k) {
        rc = launch_composite(ws.rgb_f + (size_t)k * R * nt * 3, ws.sigma_f, ws.ts_f, R, nt, rgb_fine + (size_t)k * R * 3, nullptr,
                              nullptr, st);
        if (rc) return rc;
    }
    return TGTC_OK;
}

extern "C" int tgtc_restyle_rays_folded_mx(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                           const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                           size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes,
                                           float* rgb_fine, float* t_fine, void* stream) {
    TGTC_REQUIRE(K >= 1, "restyle_rays_folded_mx: need K >= 1 latents (got %d)", K);
    TGTC_REQUIRE(R >= 0 && count >= 0, "restyle_rays_folded_mx: bad argument");
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays_folded_mx: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)");
    TGTC_REQUIRE(count <= R * nt || R == 0, "restyle_rays_folded_mx: count %lld exceeds the %lld samples", (long long)count,
                 (long long)(R * nt));
    if (K * count >= ((int64_t)1 << 31) || K * R >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "restyle_rays_folded_mx: K x count >= 2^31 (fewer latents per call)");
    TGTC_REQUIRE(fine && style, "restyle_rays_folded_mx: null handle");
    TGTC_REQUIRE(fine->kind == 0 && style->kind == 1, "restyle_rays_folded_mx: fine must be a NeRF handle, style a style handle");
    if (const int rc = list_mx_handles("restyle_rays_folded_mx", fine, style)) return rc;
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && cache && rgb_fine && (workspace || count == 0), "restyle_rays_folded_mx: null pointer");
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "restyle_rays_folded_mx: cache of %zu bytes, need %zu", cache_bytes, gc.total);
    const size_t need = tgtc_restyle_folded_workspace_bytes(count, K);
    TGTC_REQUIRE(workspace_bytes >= need, "restyle_rays_folded_mx: workspace of %zu bytes, need %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* rgb_live = static_cast<float*>(workspace);
    float* folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + tgtc_restyle_workspace_bytes(count, K));
    int rc;
    // 1. the K bias tables, then fp16mx trunk + the folded style pair's fp16mx streams over the cached list (nothing to launch
    //    for an empty list)
    if (count > 0) {
        rc = style_fold_latents_impl(style, z, K, folded, st);
        if (rc) return rc;
        rc = styled_restyle_live_folded_mx_impl(fine, style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        if (rc) return rc;
    }
    // 2. every (latent, ray): the colour sums of the dense compositing kernel; a ray without live samples gets +0
    rc = launch_composite_live(gc.ray_start, gc.live, gc.w_live, rgb_live, R, nt, K, count, rgb_fine, st);
    if (rc) return rc;
    // 3. the depth image
    if (t_fine) TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, gc.t, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TGTC_OK;
}
