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
                           const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, hipStream_t st);
int nerf_forward_list_x3_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                              const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, hipStream_t st);
int nerf_sigma_list_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         const uint32_t* live, const uint32_t* n_live, float* sigma, hipStream_t st);
int nerf_sigma_list_mx_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                            const uint32_t* live, const uint32_t* n_live, float* sigma, hipStream_t st);
int nerf_screen_rays_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                          float* sigma, hipStream_t st);
int launch_compact_candidates(const float* sigma, int64_t M, float margin, uint32_t* live, uint32_t* scratch, hipStream_t st);
int launch_count_candidates(const float* sigma, int64_t M, float margin, uint32_t* scratch, hipStream_t st);
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

// Carves consecutive planes out of one buffer, each rounded up to 256 bytes: every layout below is a sequence of take()s,
// and `off` after the last one is the layout's size.
struct PlaneCarver {
    char* base;
    size_t off;
    template <typename T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += align256(count * sizeof(T));
        return p;
    }
};

struct RenderWorkspace {
    float *ts_c, *sigma_c, *rgb_c, *w_c, *ts_f, *sigma_f, *rgb_f;
    size_t total;
    RenderWorkspace(char* base, int64_t R, int nc, int nf) {
        const int nt = nc + nf;
        PlaneCarver c{base, 0};
        ts_c = c.take<float>((size_t)R * nc);
        sigma_c = c.take<float>((size_t)R * nc);
        rgb_c = c.take<float>((size_t)R * nc * 3);
        w_c = c.take<float>((size_t)R * nc);
        ts_f = c.take<float>((size_t)R * nt);
        sigma_f = c.take<float>((size_t)R * nt);
        rgb_f = c.take<float>((size_t)R * nt * 3);
        total = c.off;
    }
};

// The planes the multi-latent stylised chain uses: RenderWorkspace's without the coarse colours, rgb_f [K,R,Nc+Nf,3].
struct MultiWorkspace {
    float *ts_c, *sigma_c, *w_c, *ts_f, *sigma_f, *rgb_f;
    size_t total;
    MultiWorkspace(char* base, int64_t R, int nc, int nf, int K) {
        const int nt = nc + nf;
        PlaneCarver c{base, 0};
        ts_c = c.take<float>((size_t)R * nc);
        sigma_c = c.take<float>((size_t)R * nc);
        w_c = c.take<float>((size_t)R * nc);
        ts_f = c.take<float>((size_t)R * nt);
        sigma_f = c.take<float>((size_t)R * nt);
        rgb_f = c.take<float>((size_t)K * R * nt * 3);
        total = c.off;
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
        PlaneCarver c{base, m.total};
        w_f = c.take<float>((size_t)R * (nc + nf));
        live = c.take<uint32_t>((size_t)R * (nc + nf));
        scratch = c.take<uint32_t>(kSparseScratchBytes / sizeof(uint32_t));
        total = c.off;
    }
};
static_assert(kSparseScratchBytes % 256 == 0, "the scratch is the workspace's last plane and is not rounded up");

// A geometry cache (tgtc_geometry_pack): a 256-byte header, then t_fine [R], ray_start [R+1], live / ts_live / w_live [count],
// every plane rounded up to 256 bytes.
struct GeometryCacheLayout {
    uint32_t *header, *ray_start, *live;
    float *t, *ts_live, *w_live;
    size_t total;
    GeometryCacheLayout(char* base, int64_t R, int64_t count) {
        PlaneCarver c{base, 0};
        header = c.take<uint32_t>(64);
        t = c.take<float>((size_t)R);
        ray_start = c.take<uint32_t>((size_t)R + 1);
        live = c.take<uint32_t>((size_t)count);
        ts_live = c.take<float>((size_t)count);
        w_live = c.take<float>((size_t)count);
        total = c.off;
    }
};

// ---- the guards the entry points share; `who` is the entry's name without tgtc_, in front of every message
constexpr int64_t kIndexLimit = (int64_t)1 << 31;   // samples, colours and list entries are indexed by 32 bits

enum : unsigned {
    kFold = 1,    // frame-constant latents z [K,32], folded into K bias tables at the end of the workspace
    kMx = 2,      // the fp16mx form of the entry (its own rule for the handles' precisions, its own launch)
    kPlane = 4,   // a restyle from the trunk plane: no NeRF handle
    kChain = 8,   // the chain geometry: the ray-only half from the plain chain's passes, screened where the handles say so
};

// the reference dereferences None when N_samples_fine == 0; require it instead
static int sample_counts(int n_coarse, int n_fine) {
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    return TGTC_OK;
}

static int samples_indexable(const char* who, int64_t R, int nt) {
    if (R * nt >= kIndexLimit) return fail(TGTC_ERR_UNSUPPORTED, "%s: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)", who);
    return TGTC_OK;
}

static int colours_indexable(const char* who, int K, int64_t R, int nt) {
    if (R >= kIndexLimit || R * nt >= kIndexLimit || R * nt * K >= kIndexLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: K x R x (n_coarse + n_fine) >= 2^31 (chunk the rays)", who);
    return TGTC_OK;
}

static int latents_indexable(const char* who, int K, int64_t R, int64_t count) {
    if (K * count >= kIndexLimit || K * R >= kIndexLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: K x count >= 2^31 (fewer latents per call)", who);
    return TGTC_OK;
}

// The rule of the fp16x3+fp16mx pair without a plane (csrc/mlp_list_mx.hip): a fine handle in TGTC_PREC_FP16_FP6 and an
// fp16x3 style handle with mx streams.
static int list_mx_handles(const char* who, const tgtc_net* fine, const tgtc_net* style) {
    if (fine->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the NeRF handle must be in fp16mx (the siblings without _mx take fp16x3 and fp16)", who);
    if (style->precision != TGTC_PREC_FP16X3)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle must be in fp16x3 (an fp16 pair has no lo halves)", who);
    if (!(style->mx && style->mx->dev))
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle has no fp16mx streams (tgtc_style_enable_mx)", who);
    return TGTC_OK;
}
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

// ONE launch of the depths-only instance of the plain ray kernel (render_fused.hip): coarse depths -> coarse sigma -> weights ->
// fine depths ts_out [R, n_coarse + n_fine], no image.  The caller has checked ray_kernel_built for the coarse precision.
static int depths_only(const tgtc_net* coarse, const double* rays_o, const double* rays_d, int64_t R, int n_coarse, int n_fine,
                       float near_, float far_, const float* jitter, float* ts_out, void* stream) {
    FusedArgs a{rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, coarse->dev, coarse->dev, nullptr, nullptr, ts_out};
    return launch_fused_depths(coarse->precision, a, as_stream(stream));
}

// That launch as an entry of its own: what the stylised chain, the multi-latent, the
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
    return depths_only(coarse, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, ts_out, stream);
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

// The geometry half of a stylised render that wants no coarse image: the fine depths ws.ts_f from the coarse net alone.
// Where the plain ray kernel is built for the coarse precision it is that kernel's first half (coarse depths -> coarse
// sigma -> weights -> fine depths, which never leave the kernel: ws.ts_c / sigma_c / w_c stay unwritten); otherwise coarse
// depths, the sigma-only NeRF launch and the per-ray stage above.  WS: any workspace with ts_c, sigma_c, w_c and ts_f.
template <class WS>
static int fine_depths(const tgtc_net* coarse, const double* rays_o, const double* rays_d, int64_t R, int n_coarse, int n_fine,
                       float near_, float far_, const float* jitter, const WS& ws, void* stream) {
    hipStream_t st = as_stream(stream);
    if (ray_kernel_built(coarse->precision, coarse->precision, -1, n_coarse, n_fine, 0))
        return depths_only(coarse, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, ws.ts_f, stream);
    int rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
    if (rc) return rc;
    rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, nullptr, ws.sigma_c, st);
    if (rc) return rc;
    return coarse_to_fine(nullptr, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, nullptr, nullptr, ws.ts_f, st);
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

// ---- the density screen of the two passes of the plain chain
// All a frame takes from a density is relu(sigma): a sample with sigma <= 0 has alpha 0 and weight +0 exactly, in the coarse
// weights that feed the inverse CDF as in the fine composite, so for such a sample only the sign of sigma matters.  A handle
// with a screen (tgtc_net_enable_screen) carries its weights in fp16 as well, and a margin m that bounds
// |sigma_screen - sigma_exact| with a factor to spare.  A screened pass is: the fp16 sigma-only launch over all samples, the
// compaction of the CANDIDATES (screen density not <= -m; NaN is one), the pass's exact kernel over that list alone.  A
// sample the list leaves out has sigma_exact < sigma_screen + m <= 0: its plane entry (the screen's value) and its exact
// density have the same relu(), and the frame has the bits of the dense pass.
// With candidate share C, p the screen launch, c the pass's dense exact launch and l the list launch per listed sample times
// the samples of the pass: p + C l + launches against c (coarse; l = 1.03 c), against today's fine pass F (fine; l the FULL
// list launch, density and colour) -- a gain while C < C*.  Measured on the MI355X (tools/time_density_screen.py --step0,
// profiles/screen_stream_timing.json "step0"; the screen launch is the four-tile stream of mlp_nerf_fp16s.hip) on the depths
// of a real 400 x 400 render at 128 + 64:
//   coarse: p = 12.77 ms, c = 38.42 ms, the list launch 1.932 ns per listed sample (l = 39.57 ms): C* = (c - p) / l = 0.648
//           (1 - p / c = 0.668).  The candidate share over the benchmark's orbit (spiral_pose 0 .. 119) is 0.261 .. 0.337:
//           its whole spread, 0.076, lets the statistic come from ANY frame of the orbit; the two compaction kernels, the
//           statistic's kernel and copy cost 0.2 ms of l, 0.005.  0.648 - 0.076 - 0.005 = 0.56.
//   fine:   p = 19.12 ms, F = 44.35 ms (the stashed two-phase pass with its compositor), the full list launch 1.689 ns per
//           listed sample (l = 51.87 ms): C* = (F - p) / l = 0.486.  Candidate share over the orbit 0.112 .. 0.142, spread
//           0.030; the extra launches (compaction, two statistics) 0.3 ms of l, 0.005.  0.486 - 0.030 - 0.005 = 0.45.
// (With the CfgFast screen launch of profiles/density_screen_timing.json, on a slower device: p = 14.42 of c = 41.20 and
// 21.66 of F = 47.17 ms, thresholds 0.55 and 0.42.)
// Both thresholds clear the orbit's shares (0.337 and 0.142) by a wide margin: AUTO screens both passes of the benchmark's
// frames once a share has landed.
constexpr float kScreenCoarseThreshold = 0.56f;
constexpr float kScreenFineThreshold = 0.45f;
// Pass 2, the sigma-only fine pass of the chain geometry (fine_sigma_pass below): there is no colour phase, so the
// break-even is another one -- the screen launch plus C x the SIGMA list launch against the dense sigma-only launch s,
// C* = (s - p) / l -- derived by the same recipe.  Measured on the MI355X (tools/time_screen_geometry.py --step0,
// profiles/screen_geometry_timing.json "step0") on the fine depths of a real 400 x 400 render (pose 5) at 128 + 64, for both
// precisions a fine handle is screened in:
//   fp16mx: p = 18.89 ms, s = 42.85 ms, the sigma list launch (nerf_mx2_kernel<IN_LIST, false>) 1.423 ns per listed sample
//           (l = 43.73 ms): C* = 0.548.  Candidate share over the orbit (spiral_pose 0 .. 119) 0.112 .. 0.142, spread 0.030;
//           the extra launches (two compaction kernels, the statistic's kernel and copy: the 0.3 ms of the fine pass above is
//           an upper bound, and the dense form takes its statistic too) 0.007 of l.  0.548 - 0.030 - 0.007 = 0.51.
//   fp16x3: p = 18.76 ms, s = 58.33 ms, the sigma list launch (nerf_x3s_kernel<IN_LIST>) 1.976 ns per listed sample
//           (l = 60.71 ms): C* = 0.652.  Orbit 0.113 .. 0.143, spread 0.030; launches 0.005.  0.652 - 0.030 - 0.005 = 0.61.
// The precisions differ; pass 2 keeps the smaller threshold for both.  It clears the orbit's share (0.143) by a wide margin:
// AUTO screens the sigma-only fine pass of the benchmark's frames once a share has landed.
constexpr float kScreenFineSigmaThreshold = 0.51f;
// Pass 3, the two-phase fine pass of a fine handle in fp16x3 (fine_pass below, TGTC_CULL_ON only): the screen
// launch plus C x the FULL fp16x3 list launch (nerf_x3_list_kernel, density and colour) against the dense full launch c,
// C* = (c - p) / l, by the same recipe.  Measured on the MI355X (tools/time_plain_x3.py --step0,
// profiles/plain_x3_two_phase_timing.json "step0") on the fine depths of a real 400 x 400 render (pose 0) at 128 + 64, both
// handles in fp16x3:
//   p = 18.92 ms, c = 73.43 ms, the full list launch 2.460 ns per listed sample (l = 75.58 ms): C* = (c - p) / l = 0.721.
//   Candidate share over the orbit (spiral_pose 0 .. 119) 0.112 .. 0.142, spread 0.030; the extra launches (compaction, two
//   statistics) 0.3 ms of l, 0.005.  0.721 - 0.030 - 0.005 = 0.68.
// (The unscreened form, for the record: the dense sigma-only launch s = 58.77 ms, so L* = (c - s) / l = 0.196 on the live share,
// 0.098 .. 0.127 over the orbit.  No AUTO rule is built on it: the pass runs under TGTC_CULL_ON only.)
constexpr float kScreenFineX3Threshold = 0.68f;

static bool screen_enabled(const tgtc_net* net) { return net->screen && net->screen->dev && net->screen->landed; }

// Does a list of up to M sample indices and the compaction's scratch fit `bytes` of dead planes?
extern "C" int tgtc_screen_list_fits(size_t bytes, int64_t M) {
    return M >= 0 && M < ((int64_t)1 << 31) && bytes >= (size_t)M * 4 + kSparseScratchBytes;
}

// AUTO's rule, pure host code: screen iff a share has landed and lies below the threshold of the pass (0: coarse, 1: fine,
// 2: the sigma-only fine pass of the chain geometry, 3: the two-phase fine pass of a fine handle in fp16x3)
extern "C" int tgtc_screen_auto_decision(int pass, uint32_t candidates, uint32_t total) {
    const float thr = pass == 0   ? kScreenCoarseThreshold
                      : pass == 2 ? kScreenFineSigmaThreshold
                      : pass == 3 ? kScreenFineX3Threshold
                                  : kScreenFineThreshold;
    return total != 0 && candidates <= total && (double)candidates < (double)thr * (double)total;
}

static bool screen_wanted(const tgtc_screen_state* s, int pass) {
    if (s->mode != TGTC_SCREEN_AUTO) return s->mode == TGTC_SCREEN_ON;
    const uint64_t word = *s->landed;   // read without waiting, as cull_wanted reads its word
    return tgtc_screen_auto_decision(pass, (uint32_t)word, (uint32_t)(word >> 32));
}

// (count, M) of the counts in `scratch` -> a handle's pinned word, asynchronously; the next render's AUTO reads what landed
static int land_share(uint32_t* scratch, int64_t M, volatile uint64_t* landed, hipStream_t st) {
    const uint32_t* stat = nullptr;
    const int rc = launch_live_stat(scratch, M, &stat, st);
    if (rc) return rc;
    TGTC_HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t*>(landed), stat, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return TGTC_OK;
}

// The coarse pass of a plain chain render that wants no coarse image: sigma_c alone.  Screened where the coarse handle (fp16x3)
// has a screen and its policy says so: the list and the 8 KiB of scratch live in the fine colour plane, which nothing uses
// before the fine pass; where they do not fit, the pass is dense.  WS: any workspace with ts_c, sigma_c and rgb_f.
template <class WS>
static int coarse_sigma_pass(const tgtc_net* coarse, const double* rays_o, const double* rays_d, int64_t R, int nc,
                             const WS& ws, size_t rgb_f_bytes, hipStream_t st) {
    const int64_t M = R * (int64_t)nc;
    tgtc_screen_state* const sc = coarse->precision == TGTC_PREC_FP16X3 && screen_enabled(coarse) ? coarse->screen : nullptr;
    char* const spare = reinterpret_cast<char*>(ws.rgb_f);
    if (sc && tgtc_screen_list_fits(rgb_f_bytes, M) && screen_wanted(sc, 0)) {
        uint32_t* const live = reinterpret_cast<uint32_t*>(spare);
        uint32_t* const scratch = reinterpret_cast<uint32_t*>(spare + (size_t)M * 4);
        int rc = nerf_screen_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, nc, ws.sigma_c, st);
        if (rc) return rc;
        rc = launch_compact_candidates(ws.sigma_c, M, sc->margin, live, scratch, st);
        if (rc) return rc;
        rc = nerf_sigma_list_impl(coarse, rays_o, rays_d, ws.ts_c, R, nc, live, scratch, ws.sigma_c, st);
        if (rc) return rc;
        ++sc->screened;
        return land_share(scratch, M, sc->landed, st);
    }
    int rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, nc, nullptr, ws.sigma_c, st);
    if (rc) return rc;
    if (sc) {
        ++sc->dense;
        if (sc->mode != TGTC_SCREEN_OFF && M < ((int64_t)1 << 31) && rgb_f_bytes >= kSparseScratchBytes) {
            uint32_t* const scratch = reinterpret_cast<uint32_t*>(spare);
            rc = launch_count_candidates(ws.sigma_c, M, sc->margin, scratch, st);
            if (rc) return rc;
            return land_share(scratch, M, sc->landed, st);
        }
    }
    return TGTC_OK;
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
    // a fine handle in fp16x3 takes the two-phase family only where the caller asks for it (TGTC_CULL_ON): no break-even
    // against its dense pass has chosen a threshold for AUTO, under which (as under OFF) the pass is what it always was
    const bool x3 = c && fine->precision == TGTC_PREC_FP16X3 && c->mode == TGTC_CULL_ON;
    const bool listable = c && (fine->precision == TGTC_PREC_FP16_FP6 || x3) && M < ((int64_t)1 << 31);
    const bool fits = listable && tgtc_screen_list_fits(dead_bytes, M);
    // the screen belongs to the two-phase family: TGTC_CULL_OFF switches it off with the rest
    tgtc_screen_state* const sc = listable && c->mode != TGTC_CULL_OFF && screen_enabled(fine) ? fine->screen : nullptr;
    const bool screen = sc && fits && screen_wanted(sc, x3 ? 3 : 1);
    const bool cull = screen || (fits && cull_wanted(c));
    // the full network over a list, in the handle's precision (fp16x3 carries no stash: tgtc_net_set_stash refuses it)
    const auto list_launch = x3 ? nerf_forward_list_x3_impl : nerf_forward_list_impl;
    uint32_t* scratch = nullptr;
    int rc;
    if (screen) {
        // the screened form: fp16 densities of all samples, the candidates' list, density AND colour of the candidates from
        // the full list launch; a sample the list leaves out keeps its screen density, which is <= -margin < 0 as its exact
        // one is below 0: relu() of either is the same +0
        uint32_t* const live = reinterpret_cast<uint32_t*>(dead);
        scratch = reinterpret_cast<uint32_t*>(dead + (size_t)M * 4);
        rc = nerf_screen_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ws.sigma_f, st);
        if (rc) return rc;
        rc = launch_compact_candidates(ws.sigma_f, M, sc->margin, live, scratch, st);
        if (rc) return rc;
        rc = list_launch(fine, rays_o, rays_d, ws.ts_f, R, nt, live, scratch, ws.rgb_f, ws.sigma_f, st);
        if (rc) return rc;
        ++c->culled, ++sc->screened;
    } else if (cull && fine->stash) {
        // the stashed form (mlp_nerf_mx2_stash.hip): the density launch parks layer 7's output of its live samples, the
        // heads-only launch reads it back; live samples that found their wave's region full are the list of the list launch
        // (which runs its prologue alone when there are none).  The per-wave counts are the statistic's parts.
        uint32_t* const ovf = reinterpret_cast<uint32_t*>(dead);
        scratch = reinterpret_cast<uint32_t*>(dead + (size_t)M * 4);
        rc = nerf_stash_fill_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ws.sigma_f, scratch, ovf, st);
        if (rc) return rc;
        rc = nerf_stash_heads_impl(fine, rays_o, rays_d, R, nt, scratch, ws.rgb_f, st);
        if (rc) return rc;
        rc = nerf_forward_list_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, ovf, scratch, ws.rgb_f, nullptr, st);
        if (rc) return rc;
        ++c->culled;
    } else if (cull) {
        uint32_t* const live = reinterpret_cast<uint32_t*>(dead);
        scratch = reinterpret_cast<uint32_t*>(dead + (size_t)M * 4);
        rc = nerf_forward_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, nullptr, ws.sigma_f, st);
        if (rc) return rc;
        rc = launch_compact_live(ws.sigma_f, M, 0.0f, live, scratch, nullptr, st);
        if (rc) return rc;
        rc = list_launch(fine, rays_o, rays_d, ws.ts_f, R, nt, live, scratch, ws.rgb_f, nullptr, st);
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
    if (screen) {
        // the scratch holds the candidates' counts: they land first, then the live statistic is taken as the dense pass
        // takes it (sigma_f > 0 holds for the same samples as in a dense plane), in the same scratch
        rc = land_share(scratch, M, sc->landed, st);
        if (rc) return rc;
        rc = launch_count_live(ws.sigma_f, M, 0.0f, scratch, st);
        if (rc) return rc;
    }
    if (scratch) {
        // (live count, M) -> the handle's pinned word, asynchronously; the next render's AUTO reads whatever has landed
        rc = land_share(scratch, M, c->landed, st);
        if (rc) return rc;
    }
    if (sc && !screen) {
        // the candidate share of a pass that was not screened: the count kernel at -margin over the exact densities
        if (scratch) {
            rc = launch_count_candidates(ws.sigma_f, M, sc->margin, scratch, st);
            if (rc) return rc;
            rc = land_share(scratch, M, sc->landed, st);
            if (rc) return rc;
        }
        ++sc->dense;
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
    if (rgb_coarse || t_coarse) rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, rgb_c, ws.sigma_c, st);
    else rc = coarse_sigma_pass(coarse, rays_o, rays_d, R, n_coarse, ws, (size_t)R * (n_coarse + n_fine) * 3 * sizeof(float), st);
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
    if (!want_coarse) {
        rc = fine_depths(coarse, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, ws, stream);
    } else {
        // the coarse image: the stylised colours on the coarse pass too (the depth image alone needs sigma only), and the
        // compositor between the passes
        rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
        if (rc) return rc;
        float* rgb_c = rgb_coarse ? ws.rgb_c : nullptr;
        if (rgb_c)
            rc = styled_forward_rays_impl(coarse, style, rays_o, rays_d, ws.ts_c, z, R, n_coarse, rgb_c, ws.sigma_c, st);
        else
            rc = nerf_forward_rays_impl(coarse, rays_o, rays_d, ws.ts_c, R, n_coarse, nullptr, ws.sigma_c, st);
        if (rc) return rc;
        rc = coarse_to_fine(rgb_c, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, rgb_coarse, t_coarse, ws.ts_f, st);
    }
    if (rc) return rc;
    // styled fine pass + composite
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
    if (const int rc = sample_counts(n_coarse, n_fine)) return rc;
    TGTC_REQUIRE(fine->precision == style->precision,
                 "render_rays_styled_multi: fine NeRF and style nets were packed with different precisions");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "render_rays_styled_multi: null pointer");
    const int nt = n_coarse + n_fine;
    if (const int rc = colours_indexable("render_rays_styled_multi", K, R, nt)) return rc;
    MultiWorkspace ws(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    TGTC_REQUIRE(workspace_bytes >= ws.total, "render_rays_styled_multi: workspace of %zu bytes, need %zu", workspace_bytes,
                 ws.total);
    hipStream_t st = as_stream(stream);
    int rc = fine_depths(coarse, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, ws, stream);
    if (rc) return rc;
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

// The sigma-only fine pass of the chain geometry: sigma_f of every fine sample, nothing else.  Screened where the fine handle
// (fp16x3 or fp16mx) has a screen and its policy says so (pass 2 of tgtc_screen_auto_decision; no colour phase exists here,
// so the cull mode has no say): fp16 densities of all samples, the candidates' list, their exact densities from the sigma
// list launch of the handle's precision.  The list and the scratch are sw.live / sw.scratch, which the compaction at
// min_weight overwrites afterwards: they always fit.  Screened or dense, the candidate share lands in the handle's pinned word.
static int fine_sigma_pass(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int nt,
                           const SparseWorkspace& sw, hipStream_t st) {
    const int64_t M = R * (int64_t)nt;
    const bool listable = (fine->precision == TGTC_PREC_FP16X3 || fine->precision == TGTC_PREC_FP16_FP6) && M < kIndexLimit;
    tgtc_screen_state* const sc = listable && screen_enabled(fine) ? fine->screen : nullptr;
    int rc;
    if (sc && screen_wanted(sc, 2)) {
        rc = nerf_screen_rays_impl(fine, rays_o, rays_d, sw.m.ts_f, R, nt, sw.m.sigma_f, st);
        if (rc) return rc;
        rc = launch_compact_candidates(sw.m.sigma_f, M, sc->margin, sw.live, sw.scratch, st);
        if (rc) return rc;
        rc = (fine->precision == TGTC_PREC_FP16_FP6 ? nerf_sigma_list_mx_impl : nerf_sigma_list_impl)(
            fine, rays_o, rays_d, sw.m.ts_f, R, nt, sw.live, sw.scratch, sw.m.sigma_f, st);
        if (rc) return rc;
        ++sc->screened;
        return land_share(sw.scratch, M, sc->landed, st);
    }
    rc = nerf_forward_rays_impl(fine, rays_o, rays_d, sw.m.ts_f, R, nt, nullptr, sw.m.sigma_f, st);
    if (rc) return rc;
    if (sc) {
        ++sc->dense;
        if (sc->mode != TGTC_SCREEN_OFF) {
            rc = launch_count_candidates(sw.m.sigma_f, M, sc->margin, sw.scratch, st);
            if (rc) return rc;
            return land_share(sw.scratch, M, sc->landed, st);
        }
    }
    return TGTC_OK;
}

// Steps 1-4 of the culled stylised render, the half that depends on the ray alone (tgtc_render_rays_styled_sparse and
// tgtc_geometry_build): fine depths ts_f, sigma_f, the depth image, the weights plane w_f, the ascending list live[] of the
// samples with w_f > min_weight and its length (scratch word 0, and *live_count where given).
// chain: steps 1 and 2 are the PLAIN CHAIN's passes (tgtc_render_rays_plain without a coarse image) -- coarse depths, the coarse
// sigma pass, the per-ray stage, the sigma-only fine pass -- each screened where its handle's policy says so; the coarse list
// lives in the first colour plane, which nothing uses before step 5.  The depths are those of the plain chain bit for bit,
// and agree with the ray kernel's first half (chain = false) only to rounding: the caller asks for one or the other.
static int ray_geometry(bool chain, const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d,
                        int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter, float min_weight,
                        const SparseWorkspace& sw, float* t_fine, uint32_t* live_count, void* stream) {
    const MultiWorkspace& ws = sw.m;
    const int nt = n_coarse + n_fine;
    hipStream_t st = as_stream(stream);
    int rc;
    if (chain) {
        rc = tgtc_sample_coarse(rays_o, rays_d, R, n_coarse, near_, far_, jitter, nullptr, ws.ts_c, stream);
        if (rc) return rc;
        rc = coarse_sigma_pass(coarse, rays_o, rays_d, R, n_coarse, ws, (size_t)R * nt * 3 * sizeof(float), st);
        if (rc) return rc;
        rc = coarse_to_fine(nullptr, ws.sigma_c, ws.ts_c, ws.w_c, rays_o, rays_d, R, n_coarse, n_fine, nullptr, nullptr, ws.ts_f, st);
        if (rc) return rc;
        rc = fine_sigma_pass(fine, rays_o, rays_d, R, nt, sw, st);
        if (rc) return rc;
    } else {
        // 1. geometry half, as tgtc_render_rays_styled_multi
        rc = fine_depths(coarse, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, ws, stream);
        if (rc) return rc;
        // 2. sigma of every fine sample (the sigma-only NeRF launch carries the bits of the styled kernels' sigma:
        //    tests/test_sparse_style_gpu.py, test_sigma_pass_bits_of_the_styled_kernel)
        rc = nerf_forward_rays_impl(fine, rays_o, rays_d, ws.ts_f, R, nt, nullptr, ws.sigma_f, st);
        if (rc) return rc;
    }
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
//
// The body of the three tgtc_render_rays_styled_sparse* entries.  flags: 0 is the per-ray form, z [K,R,32]; kFold the
// frame-constant one, z [K,32] folded into K bias tables in one more plane at the end of the workspace; kFold | kMx that
// for the fp16x3+fp16mx pair.  They differ in the rule for the handles' precisions and in the list launch, nothing else.
// kChain on top of any of the three: the chain geometry (ray_geometry), tgtc_render_rays_styled_sparse_chain.
static int render_rays_culled(const char* who, unsigned flags, const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                              const double* rays_o, const double* rays_d, const float* z, int K, int64_t R, int n_coarse,
                              int n_fine, float near_, float far_, const float* jitter, float min_weight, void* workspace,
                              size_t workspace_bytes, float* rgb_fine, float* t_fine, uint32_t* live_count, void* stream) {
    const bool fold = flags & kFold, mx = flags & kMx;
    TGTC_REQUIRE(K >= 1, "%s: need K >= 1 %s (got %d)", who, fold ? "latents" : "latent sets", K);
    TGTC_REQUIRE(min_weight >= 0.0f, "%s: min_weight must be >= 0 and not NaN (got %g)", who, (double)min_weight);
    TGTC_REQUIRE(R >= 0, "%s: bad argument", who);
    if (const int rc = sample_counts(n_coarse, n_fine)) return rc;
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (const int rc = colours_indexable(who, K, R, nt)) return rc;
    TGTC_REQUIRE(coarse && fine && style, "%s: null handle", who);
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0 && style->kind == 1,
                 "%s: coarse and fine must be NeRF handles, style a style handle", who);
    if (mx) {
        if (const int rc = list_mx_handles(who, fine, style)) return rc;
    } else {
        TGTC_REQUIRE(fine->precision == style->precision, "%s: fine NeRF and style nets were packed with different precisions", who);
    }
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && workspace && rgb_fine && t_fine, "%s: null pointer", who);
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, K);
    const size_t need = sw.total + (fold ? align256(tgtc_style_folded_bytes(K)) : 0);
    TGTC_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
    float* folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + sw.total);
    const MultiWorkspace& ws = sw.m;
    hipStream_t st = as_stream(stream);
    int rc;
    // 0. the K bias tables
    if (fold) {
        rc = style_fold_latents_impl(style, z, K, folded, st);
        if (rc) return rc;
    }
    // 1-4. everything that depends on the ray alone
    rc = ray_geometry(flags & kChain, coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, t_fine,
                      live_count, stream);
    if (rc) return rc;
    // 5. dead samples keep colour +0
    TGTC_HIP_CHECK(hipMemsetAsync(ws.rgb_f, 0, (size_t)K * R * nt * 3 * sizeof(float), st));
    // 6. over the list (the host never learns its length): trunk + concat MLP + style MLP, their folded forms, or the
    //    fp16mx trunk + the folded style pair's fp16mx streams
    if (mx) rc = styled_forward_list_folded_mx_impl(fine, style, rays_o, rays_d, ws.ts_f, folded, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    else if (fold) rc = styled_forward_list_folded_impl(fine, style, rays_o, rays_d, ws.ts_f, folded, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    else rc = styled_forward_rays_sparse_impl(fine, style, rays_o, rays_d, ws.ts_f, z, K, R, nt, sw.live, sw.scratch, ws.rgb_f, st);
    if (rc) return rc;
    // 7. compositing over the shared sigma / depths
    for (int k = 0; k < K; ++k) {
        rc = launch_composite(ws.rgb_f + (size_t)k * R * nt * 3, ws.sigma_f, ws.ts_f, R, nt, rgb_fine + (size_t)k * R * 3, nullptr,
                              nullptr, st);
        if (rc) return rc;
    }
    return TGTC_OK;
}

extern "C" int tgtc_render_rays_styled_sparse(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                              const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                              int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                              float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                              float* t_fine, uint32_t* live_count, void* stream) {
    return render_rays_culled("render_rays_styled_sparse", 0, coarse, fine, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, near_,
                              far_, jitter, min_weight, workspace, workspace_bytes, rgb_fine, t_fine, live_count, stream);
}

// ------------------------------------------------------------------------------------------------ geometry cache + restyle
// The ray-only half of the culled render kept as a compact device buffer, and "the same rays under new latents" from it:
// one launch of the compact indexed kernel over the cached list, one compositing launch over (latent, ray).

// Steps 1-4 of tgtc_render_rays_styled_sparse on the sparse workspace at K = 1.  The depth image also stays in the
// workspace (the first R floats of the colour plane, which no step of the build uses), where tgtc_geometry_pack reads it.
// The body of tgtc_geometry_build and (chain) tgtc_geometry_build_chain.
static int geometry_build(const char* who, bool chain, const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o,
                          const double* rays_d, int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                          float min_weight, void* workspace, size_t workspace_bytes, float* t_fine, uint32_t* live_count,
                          void* stream) {
    TGTC_REQUIRE(min_weight >= 0.0f, "%s: min_weight must be >= 0 and not NaN (got %g)", who, (double)min_weight);
    TGTC_REQUIRE(coarse && fine && R >= 0, "%s: bad argument", who);
    TGTC_REQUIRE(coarse->kind == 0 && fine->kind == 0, "%s: coarse and fine must be NeRF handles", who);
    TGTC_REQUIRE(n_coarse >= 3 && n_fine >= 1, "render: need n_coarse >= 3 and n_fine >= 1 (got %d, %d)", n_coarse, n_fine);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && workspace && live_count, "%s: null pointer", who);
    const int nt = n_coarse + n_fine;
    if (R * nt >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "%s: R x (n_coarse + n_fine) >= 2^31 (chunk the rays)", who);
    SparseWorkspace sw(static_cast<char*>(workspace), R, n_coarse, n_fine, 1);
    TGTC_REQUIRE(workspace_bytes >= sw.total, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, sw.total);
    int rc = ray_geometry(chain, coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight, sw, sw.m.rgb_f,
                          live_count, stream);
    if (rc) return rc;
    if (t_fine)
        TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, sw.m.rgb_f, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return TGTC_OK;
}

extern "C" int tgtc_geometry_build(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d,
                                   int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                   float min_weight, void* workspace, size_t workspace_bytes, float* t_fine,
                                   uint32_t* live_count, void* stream) {
    return geometry_build("geometry_build", false, coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter, min_weight,
                          workspace, workspace_bytes, t_fine, live_count, stream);
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

extern "C" size_t tgtc_restyle_folded_workspace_bytes(int64_t count, int K) {
    if (count < 0 || K < 1) return 0;
    return tgtc_restyle_workspace_bytes(count, K) + align256(tgtc_style_folded_bytes(K));
}

// The body of the six tgtc_restyle_rays* entries: one style launch over the cached list into the compact colour planes, one
// compositing launch over (latent, ray), the depth copy.  flags: kFold as in render_rays_culled; kPlane reads the fine NeRF
// trunk from the plane of tgtc_geometry_trunk (below) and takes no NeRF handle (fine is not looked at), the other forms
// take no plane (trunk is not looked at); kMx runs the style networks on the handle's fp16mx streams -- from the plane, or
// behind an fp16mx fine handle -- and exists folded only.  The forms differ in the rule for the handles and in the style launch.
static int restyle_rays(const char* who, unsigned flags, const tgtc_net* fine, const tgtc_net* style, const double* rays_o,
                        const double* rays_d, const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                        size_t cache_bytes, int64_t count, const void* trunk, size_t trunk_bytes, void* workspace,
                        size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream) {
    const bool fold = flags & kFold, mx = flags & kMx, plane = flags & kPlane;
    TGTC_REQUIRE(K >= 1, "%s: need K >= 1 %s (got %d)", who, fold || plane ? "latents" : "latent sets", K);
    TGTC_REQUIRE(R >= 0 && count >= 0, "%s: bad argument", who);
    if (const int rc = sample_counts(n_coarse, n_fine)) return rc;
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (const int rc = samples_indexable(who, R, nt)) return rc;
    TGTC_REQUIRE(count <= R * nt || R == 0, "%s: count %lld exceeds the %lld samples", who, (long long)count, (long long)(R * nt));
    if (const int rc = latents_indexable(who, K, R, count)) return rc;
    TGTC_REQUIRE(style && (plane || fine), "%s: null handle", who);
    if (plane) {
        TGTC_REQUIRE(style->kind == 1, "%s: style must be a style handle", who);
        if (mx && !(style->mx && style->mx->dev))
            return fail(TGTC_ERR_UNSUPPORTED, "%s: the style handle has no fp16mx streams (tgtc_style_enable_mx)", who);
    } else {
        TGTC_REQUIRE(fine->kind == 0 && style->kind == 1, "%s: fine must be a NeRF handle, style a style handle", who);
        if (mx) {
            if (const int rc = list_mx_handles(who, fine, style)) return rc;
        } else {
            TGTC_REQUIRE(fine->precision == style->precision, "%s: fine NeRF and style nets were packed with different precisions", who);
        }
    }
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && z && cache && rgb_fine && (workspace || count == 0) && (!plane || trunk || count == 0),
                 "%s: null pointer", who);
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "%s: cache of %zu bytes, need %zu", who, cache_bytes, gc.total);
    if (plane) {
        const size_t need_plane = tgtc_geometry_trunk_bytes(style->precision, count);
        TGTC_REQUIRE(trunk_bytes >= need_plane, "%s: plane of %zu bytes, need %zu", who, trunk_bytes, need_plane);
    }
    const size_t need = fold ? tgtc_restyle_folded_workspace_bytes(count, K) : tgtc_restyle_workspace_bytes(count, K);
    TGTC_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* rgb_live = static_cast<float*>(workspace);
    int rc;
    // 1. (the K bias tables, then) the trunk -- computed, or base_remap from the plane -- + concat MLP + style MLP over the
    //    cached list (nothing to launch for an empty list)
    if (count > 0) {
        float* folded = nullptr;
        if (fold) {
            folded = reinterpret_cast<float*>(static_cast<char*>(workspace) + tgtc_restyle_workspace_bytes(count, K));
            rc = style_fold_latents_impl(style, z, K, folded, st);
            if (rc) return rc;
        }
        if (plane && mx) rc = styled_restyle_plane_mx_impl(style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, trunk, rgb_live, st);
        else if (plane) rc = styled_restyle_plane_impl(style, rays_o, rays_d, z, folded, K, R, nt, gc.live, gc.ts_live, count, trunk, rgb_live, st);
        else if (mx) rc = styled_restyle_live_folded_mx_impl(fine, style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        else if (fold) rc = styled_restyle_live_folded_impl(fine, style, rays_o, rays_d, folded, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        else rc = styled_restyle_live_impl(fine, style, rays_o, rays_d, z, K, R, nt, gc.live, gc.ts_live, count, rgb_live, st);
        if (rc) return rc;
    }
    // 2. every (latent, ray): the colour sums of the dense compositing kernel; a ray without live samples gets +0
    rc = launch_composite_live(gc.ray_start, gc.live, gc.w_live, rgb_live, R, nt, K, count, rgb_fine, st);
    if (rc) return rc;
    // 3. the depth image
    if (t_fine) TGTC_HIP_CHECK(hipMemcpyAsync(t_fine, gc.t, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TGTC_OK;
}

extern "C" int tgtc_restyle_rays(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                 const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                 size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                 float* t_fine, void* stream) {
    return restyle_rays("restyle_rays", 0, fine, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache, cache_bytes, count, nullptr,
                        0, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

// ------------------------------------------------------------------------------------------------ frame-constant latents
// The culled render and the restyle for latents that do not depend on the ray: z [K,32].  The latent k-step of every layer
// of the two style networks is folded into K bias tables (tgtc_style_fold_latents, mlp_style.hip) kept in one more plane
// at the end of the workspace, and the folded instances of the indexed kernels (mlp_style_sparse.hip) run on the streams
// packed without that k-step.  Everything else is the unfolded sibling's (kFold of the shared bodies).

// The folded list launch as an entry of its own, and (kMx) its form for the fp16x3+fp16mx pair.
static int styled_forward_list_folded(const char* who, unsigned flags, const tgtc_net* nerf, const tgtc_net* style,
                                      const double* rays_o, const double* rays_d, const float* ts, const void* folded, int K,
                                      int64_t R, int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    TGTC_REQUIRE(K >= 1, "%s: need K >= 1 latents (got %d)", who, K);
    TGTC_REQUIRE(R >= 0 && N >= 1, "%s: bad argument", who);
    if (R >= kIndexLimit || R * (int64_t)N >= kIndexLimit || R * (int64_t)N * K >= kIndexLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: K x R x N >= 2^31 in one launch (chunk the rays)", who);
    TGTC_REQUIRE(nerf && style, "%s: null handle", who);
    TGTC_REQUIRE(nerf->kind == 0 && style->kind == 1, "%s: nerf must be a NeRF handle, style a style handle", who);
    if (flags & kMx) {
        if (const int rc = list_mx_handles(who, nerf, style)) return rc;
    } else {
        TGTC_REQUIRE(nerf->precision == style->precision, "%s: NeRF and style nets were packed with different precisions", who);
    }
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && folded && live && n_live && rgb, "%s: null pointer", who);
    return (flags & kMx ? styled_forward_list_folded_mx_impl : styled_forward_list_folded_impl)(
        nerf, style, rays_o, rays_d, ts, folded, K, R, N, live, n_live, rgb, as_stream(stream));
}

extern "C" int tgtc_styled_forward_list_folded(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                               const double* rays_d, const float* ts, const void* folded, int K, int64_t R,
                                               int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    return styled_forward_list_folded("styled_forward_list_folded", 0, nerf, style, rays_o, rays_d, ts, folded, K, R, N, live, n_live,
                                      rgb, stream);
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
    return render_rays_culled("render_rays_styled_sparse_folded", kFold, coarse, fine, style, rays_o, rays_d, z, K, R, n_coarse,
                              n_fine, near_, far_, jitter, min_weight, workspace, workspace_bytes, rgb_fine, t_fine, live_count,
                              stream);
}

extern "C" int tgtc_restyle_rays_folded(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                        const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                        size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes,
                                        float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays("restyle_rays_folded", kFold, fine, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache, cache_bytes, count,
                        nullptr, 0, workspace, workspace_bytes, rgb_fine, t_fine, stream);
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

// The body of tgtc_geometry_trunk and (mx) tgtc_geometry_trunk_mx: the same arguments and checks in the same order.  The
// first takes an fp16x3 or fp16 handle and writes the plane of that precision; the second takes a handle in
// TGTC_PREC_FP16_FP6 and writes the TGTC_PREC_FP16X3 plane (csrc/mlp_trunk_mx.hip).
static int geometry_trunk(const char* who, bool mx, const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R,
                          int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count, void* trunk,
                          size_t trunk_bytes, void* stream) {
    TGTC_REQUIRE(R >= 0 && count >= 0, "%s: bad argument", who);
    if (const int rc = sample_counts(n_coarse, n_fine)) return rc;
    // (the checks that need no handle come first: they can be exercised without a device)
    const int nt = n_coarse + n_fine;
    if (const int rc = samples_indexable(who, R, nt)) return rc;
    TGTC_REQUIRE(count <= R * nt || R == 0, "%s: count %lld exceeds the %lld samples", who, (long long)count, (long long)(R * nt));
    TGTC_REQUIRE(fine, "%s: null handle", who);
    TGTC_REQUIRE(fine->kind == 0, "%s: fine must be a NeRF handle", who);
    if (mx && fine->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: built for fp16mx handles only (tgtc_geometry_trunk takes fp16x3 and fp16)", who);
    if (!mx && fine->precision != TGTC_PREC_FP16X3 && fine->precision != TGTC_PREC_FP16)
        return fail(TGTC_ERR_UNSUPPORTED, "%s: the style kernels are built for fp16x3 and fp16 handles only", who);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && cache && (trunk || count == 0), "%s: null pointer", who);
    GeometryCacheLayout gc(static_cast<char*>(const_cast<void*>(cache)), R, count);
    TGTC_REQUIRE(cache_bytes >= gc.total, "%s: cache of %zu bytes, need %zu", who, cache_bytes, gc.total);
    const size_t need = tgtc_geometry_trunk_bytes(mx ? TGTC_PREC_FP16X3 : fine->precision, count);
    TGTC_REQUIRE(trunk_bytes >= need, "%s: plane of %zu bytes, need %zu", who, trunk_bytes, need);
    if (count == 0) return TGTC_OK;
    return (mx ? styled_trunk_plane_mx_impl : styled_trunk_plane_impl)(fine, rays_o, rays_d, R, nt, gc.live, gc.ts_live, count, trunk,
                                                                       as_stream(stream));
}

extern "C" int tgtc_geometry_trunk(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                                   int n_fine, const void* cache, size_t cache_bytes, int64_t count, void* trunk,
                                   size_t trunk_bytes, void* stream) {
    return geometry_trunk("geometry_trunk", false, fine, rays_o, rays_d, R, n_coarse, n_fine, cache, cache_bytes, count, trunk,
                          trunk_bytes, stream);
}

extern "C" int tgtc_geometry_trunk_mx(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                                      int n_fine, const void* cache, size_t cache_bytes, int64_t count, void* trunk,
                                      size_t trunk_bytes, void* stream) {
    return geometry_trunk("geometry_trunk_mx", true, fine, rays_o, rays_d, R, n_coarse, n_fine, cache, cache_bytes, count, trunk,
                          trunk_bytes, stream);
}

// tgtc_restyle_rays / tgtc_restyle_rays_folded with the trunk read from the plane (kPlane of restyle_rays): the same
// workspaces, the same compositing launch and depth copy behind another style launch.
extern "C" int tgtc_restyle_rays_trunk(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z, int K,
                                       int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                                       const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                                       float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays("restyle_rays_trunk", kPlane, nullptr, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache, cache_bytes,
                        count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

extern "C" int tgtc_restyle_rays_trunk_folded(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                                              int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes,
                                              int64_t count, const void* trunk, size_t trunk_bytes, void* workspace,
                                              size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays("restyle_rays_trunk_folded", kPlane | kFold, nullptr, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache,
                        cache_bytes, count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

// ... and with the style networks in fp16mx: the folded form on the handle's mx streams (tgtc_style_enable_mx; an fp16x3 handle,
// so the plane's size is checked as the fp16x3 plane's)
extern "C" int tgtc_restyle_rays_trunk_folded_mx(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                                                 int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                                 size_t cache_bytes, int64_t count, const void* trunk, size_t trunk_bytes,
                                                 void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                                 void* stream) {
    return restyle_rays("restyle_rays_trunk_folded_mx", kPlane | kFold | kMx, nullptr, style, rays_o, rays_d, z, K, R, n_coarse,
                        n_fine, cache, cache_bytes, count, trunk, trunk_bytes, workspace, workspace_bytes, rgb_fine, t_fine, stream);
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
// tgtc_render_rays_styled_sparse_folded, tgtc_restyle_rays_folded: kMx of the same bodies); only the rule for the handles'
// precisions (list_mx_handles) and the launch differ.
extern "C" int tgtc_styled_forward_list_folded_mx(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                                  const double* rays_d, const float* ts, const void* folded, int K, int64_t R,
                                                  int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    return styled_forward_list_folded("styled_forward_list_folded_mx", kMx, nerf, style, rays_o, rays_d, ts, folded, K, R, N, live,
                                      n_live, rgb, stream);
}

extern "C" int tgtc_render_rays_styled_sparse_folded_mx(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                                        const double* rays_o, const double* rays_d, const float* z, int K,
                                                        int64_t R, int n_coarse, int n_fine, float near_, float far_,
                                                        const float* jitter, float min_weight, void* workspace,
                                                        size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                                        uint32_t* live_count, void* stream) {
    return render_rays_culled("render_rays_styled_sparse_folded_mx", kFold | kMx, coarse, fine, style, rays_o, rays_d, z, K, R,
                              n_coarse, n_fine, near_, far_, jitter, min_weight, workspace, workspace_bytes, rgb_fine, t_fine,
                              live_count, stream);
}

extern "C" int tgtc_restyle_rays_folded_mx(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                           const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache,
                                           size_t cache_bytes, int64_t count, void* workspace, size_t workspace_bytes,
                                           float* rgb_fine, float* t_fine, void* stream) {
    return restyle_rays("restyle_rays_folded_mx", kFold | kMx, fine, style, rays_o, rays_d, z, K, R, n_coarse, n_fine, cache,
                        cache_bytes, count, nullptr, 0, workspace, workspace_bytes, rgb_fine, t_fine, stream);
}

// ------------------------------------------------------------------------------------------------ the chain geometry
// The culled stylised render and the geometry build with their ray-only half taken from the plain chain's passes
// (ray_geometry, chain), each screened where its handle's policy says so (tgtc_net_set_screen).  A mode the
// caller asks for: the depths are the plain chain's, which the ray kernel's first half matches only to rounding.  The
// same bodies as the siblings, with kChain; every check, workspace and order of work is theirs.
extern "C" int tgtc_geometry_build_chain(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d,
                                         int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                         float min_weight, void* workspace, size_t workspace_bytes, float* t_fine,
                                         uint32_t* live_count, void* stream) {
    return geometry_build("geometry_build_chain", true, coarse, fine, rays_o, rays_d, R, n_coarse, n_fine, near_, far_, jitter,
                          min_weight, workspace, workspace_bytes, t_fine, live_count, stream);
}

// form: 0 the per-ray form (z [K,R,32]), 1 the folded one (z [K,32]), 2 the folded one for the fp16x3+fp16mx pair
extern "C" int tgtc_render_rays_styled_sparse_chain(int form, const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                                    const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                                    int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                                    float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                                    float* t_fine, uint32_t* live_count, void* stream) {
    TGTC_REQUIRE(form >= 0 && form <= 2, "render_rays_styled_sparse_chain: form is 0 (per ray), 1 (folded) or 2 (folded, fp16mx); got %d",
                 form);
    const unsigned flags = kChain | (form == 0 ? 0u : form == 1 ? (unsigned)kFold : (unsigned)(kFold | kMx));
    return render_rays_culled("render_rays_styled_sparse_chain", flags, coarse, fine, style, rays_o, rays_d, z, K, R, n_coarse, n_fine,
                              near_, far_, jitter, min_weight, workspace, workspace_bytes, rgb_fine, t_fine, live_count, stream);
}
