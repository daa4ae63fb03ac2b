// rtw_wavefront_dispatch.h -- the host side of the wavefront path: grid sizes, the staging plan, the launches of one
// batch and the scene-class tables.  Included as the last line of rtw_wavefront.hip (it names the kernel templates),
// so once per translation unit: rtw_wavefront.hip itself and the four RTW_WF_*_TU wrappers.
#pragma once
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

namespace {

// resident blocks of `kernel`, rounded down to whole stripes of waves
template <typename K>
uint32_t wf_grid(K kernel, int n_cu, size_t lds = 0, uint32_t threads = 256) {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kernel, (int)threads, lds) != hipSuccess || b < 1) b = 1;
    uint32_t g = (uint32_t)(b * n_cu);
    // whole sets of stripes: the grid's waves a multiple of RTW_WF_STRIPES (every stripe the same number of
    // waves, WfIter), i.e. blocks a multiple of 256 / gcd(256, waves per block)
    uint32_t wpb = threads / 64, gcd = RTW_WF_STRIPES;
    for (uint32_t a = wpb; a;) {
        const uint32_t t = gcd % a;
        gcd = a;
        a = t;
    }
    const uint32_t per = RTW_WF_STRIPES / gcd;
    g -= g % per;
    return g ? g : per;
}

// The one grid cache: wf_grid of (kernel, CU count, dynamic LDS, block size), process-wide, so the 8 Tasks of a
// render (main.zig:314-326) and contexts on devices or partitions of different sizes share the occupancy queries.
// Keyed by the CU count too: a grid larger than the device's would overflow the stripes that
// rtw_wavefront_max_waves(n_cu) sized.  (One instance per translation unit, as a kernel's host stub is.)
struct WfGridCache {
    std::mutex mu;
    std::map<std::tuple<const void*, int, size_t, uint32_t>, uint32_t> grids;
};
inline WfGridCache& wf_grid_cache() {
    static WfGridCache c;
    return c;
}
template <typename K>
uint32_t wf_grid_for(K kernel, int n_cu, size_t lds = 0, uint32_t threads = 256) {
    WfGridCache& c = wf_grid_cache();
    const auto key = std::make_tuple(reinterpret_cast<const void*>(kernel), n_cu, lds, threads);
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.grids.find(key);
    if (it == c.grids.end()) it = c.grids.emplace(key, wf_grid(kernel, n_cu, lds, threads)).first;
    return it->second;
}

// every wavefront launch
template <typename K, typename... A>
void wf_launch(K kernel, uint32_t grid, uint32_t threads, size_t lds, hipStream_t st, const A&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
}

// The runtime choices that select a template argument: f gets it as a std::integral_constant.
template <int V>
using wf_int = std::integral_constant<int, V>;
// CNT: the kernel with the counters compiled in (1) or out (0)
template <typename F>
void wf_with_cnt(const rtw_launch& L, F&& f) {
    if (L.counters) f(wf_int<1>{});
    else f(wf_int<0>{});
}
// CN: the compact-node form
template <typename F>
void wf_with_cn(int cn, F&& f) {
    if (cn == CN_F32_4) f(wf_int<CN_F32_4>{});
    else if (cn == CN_F16_4) f(wf_int<CN_F16_4>{});
    else f(wf_int<CN_F16_8>{});
}
// IT0 / CAM: iteration 0's instantiation (1: camera rays) or the later iterations' (0)
template <typename F>
void wf_with_it0(uint32_t it, F&& f) {
    if (it == 0) f(wf_int<1>{});
    else f(wf_int<0>{});
}

// dynamic LDS of the kernels that walk through L1/L2: the two-wide walk's per-lane stacks
template <uint32_t FEAT>
size_t wf_w2_lds(const rtw_launch& L) {
    if constexpr ((FEAT & (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_MOVING)) == 0) {
        if (L.w2nodes && L.fast_box) return (size_t)256u * 4u * L.w2_stack;
    }
    return 0;
}

// The camera-ray candidate lists of a batch (static sphere scenes with the compact nodes): the
// flat scan for small trees, the frustum walk for large ones.  wf_lists returns W with tl_count null when off.
template <uint32_t FEAT>
bool wf_lists_on(const rtw_launch& L, const rtw_wf& W) {
    return W.tl_count && L.cnodes && !(FEAT & (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_MOVING)) && L.max_depth != 0;
}
// one builder over the batch's tiles: the flat scan (one block per tile) or the frustum walk (one lane per tile)
void wf_build_lists(const rtw_launch& L, const rtw_wf& W, hipStream_t st, bool scan) {
    const uint32_t tiles = W.n_pix / 64u;
    if (scan) wf_launch(wf_tile_lists, tiles, 64, 0, st, L, W);
    else wf_launch(wf_tile_lists_walk, (tiles + 63u) / 64u, 64, 0, st, L, W);
}
template <uint32_t FEAT>
rtw_wf wf_lists(const rtw_launch& L, const rtw_wf& W, hipStream_t st) {
    rtw_wf Wt = W;
    if (!wf_lists_on<FEAT>(L, W)) {
        Wt.tl_count = nullptr;
        return Wt;
    }
    wf_build_lists(L, Wt, st, L.n_nodes <= 4096u);
    return Wt;
}
// rtw_debug_tile_lists: the lists of class FEAT's batch alone, by wf_lists' builder (0), the scan (1) or the walk (2);
// 0: the class renders without lists, 1: launched
template <uint32_t FEAT>
int wf_lists_only(const rtw_launch& L, const rtw_wf& W, hipStream_t st, uint32_t builder) {
    if (!wf_lists_on<FEAT>(L, W)) return 0;
    wf_build_lists(L, W, st, builder ? builder == 1u : L.n_nodes <= 4096u);
    return 1;
}

// Coherent-queue settings of a launch whose grid has nw waves.  Iteration 0 deals runs of
// up to 16 samples per tile, shorter when a wave would get fewer than 64 runs (a small batch: whole runs
// would leave the waves' shares of work uneven); direction bucketing only when a wave's iteration 0 has at
// least RTW_WF_SORT_MIN_CHUNKS chunks -- each open block ends its iteration partly dead, which only a large
// share of survivors per wave amortises (simple_light, 137 chunks per wave: -10 % with bucketing).  Deal bit 128
// (RTW_DEAL_SMALL_SORT) lifts that gate, so the tests run the bucketed queues of the large benched batches on small
// images (tests/test_gpu_parity.py, test_gpu_objects.py).
#define RTW_WF_SORT_MIN_CHUNKS 192u
rtw_wf wf_coherence(const rtw_wf& W, uint32_t nw, uint32_t sort_iters) {
    rtw_wf C = W;
    const uint32_t per_wave = nw ? (W.n_paths >> 6) / nw : 0u;
    uint32_t lg = 0;
    while (lg < 4 && (per_wave >> (lg + 1)) >= 64u) lg++;
    // the dynamic deal only where the waves have enough work to share: a small batch (simple_light, 137 chunks per
    // wave) ran 6 % slower with it -- its tail's claims cost more than they balance (profiles/r5_deal/)
    if (per_wave < RTW_WF_SORT_MIN_CHUNKS && !(C.deal_mode & 8u)) C.deal = nullptr;  // (bit 8: tests force it)
    if (C.deal && (C.deal_mode & 1u)) lg = 4;  // dynamic deal: the waves balance themselves, runs keep 16 samples
    C.run_log2 = lg;
    C.sort_iters = (per_wave >= RTW_WF_SORT_MIN_CHUNKS || (C.deal_mode & 128u)) ? sort_iters : 0u;
    return C;
}

// largest LDS stage of the wavefront trace (bytes); larger trees read L1/L2
#define RTW_WF_LDS_MAX (64u * 1024u)
#define RTW_WF_CLDS_MAX (150u * 1024u)  // compact-node LDS stage (one 1024-thread block per CU)
// scene classes whose fused step never runs on the compact LDS stage (textured scenes keep the 32-B stage: it
// leaves LDS for the Perlin tables and the 1024-thread compact kernel would spill at its 128-VGPR cap -- C5 -20 %
// measured), so no compact-LDS step or tail is instantiated for them
#define RTW_WF_NO_CLDS (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_MOVING | RTW_F_IMAGE | RTW_F_NOISE)

// Where a batch's kernels read the tree, and their dynamic LDS sizes (0 = not staged):
//   compact nodes of all orders in LDS   wf_step_clds / wf_step_clds2, wf_tail_clds*, wf_trace_clds
//   the 32-B node array in LDS           wf_step<FEAT, true>, wf_tail_lds, wf_trace<FEAT, true>
//   the tree through L1/L2               wf_step<FEAT, false>, wf_tail / wf_tail_w5, wf_trace<FEAT, false>
struct WfStage {
    bool fused;        // one wf_step* kernel per iteration (wf_run_fused), else wf_trace* + wf_shade (wf_run_split)
    int cn;            // the compact-node form (CN_*)
    size_t w2;         // the L1/L2 kernels' dynamic LDS (wf_w2_lds)
    // fused: one stage or neither
    size_t f_clds;     // compact stage: it and the 1024-thread step's push cursors within RTW_WF_CLDS_MAX
    size_t f_lds;      // else the 32-B stage, rounded to 512 B
    bool two;          // compact step and tail as two 768-thread blocks per CU (else one of 1024 threads)
    size_t f_step_clds;  // the compact step: f_clds + the materials when they fit
    size_t f_step_lds;   // wf_step<FEAT, true>: f_lds + Perlin tables + geometry + materials
    size_t f_tail_clds;  // the tail's stage (L.wf_fuse & 2): f_clds, or
    size_t f_tail_lds;   //   f_lds + geometry + materials, or neither: through L1/L2
    // split: the compact stage for the trace and the 32-B one for the tail may both be on
    size_t s_clds;       // wf_trace_clds: the compact stage alone (no cursors: the trace does not push)
    size_t s_trace_lds;  // else wf_trace<FEAT, true>: the 32-B stage + geometry
    size_t s_tail_lds;   // wf_tail_lds (L.wf_fuse & 2): s_trace_lds + materials, whichever stage the trace used
};

template <uint32_t FEAT>
WfStage wf_stage(const rtw_launch& L) {
    // (the fused steps' push cursors are static LDS on top of the dynamic sizes here: at 1024 threads, at 768)
    constexpr size_t cur1 = RTW_WF_CURSOR_BYTES(1024u), cur2 = RTW_WF_CURSOR_BYTES(768u);
    WfStage P{};
    P.cn = L.cnode32 ? CN_F32_4 : L.n_orders == 4 ? CN_F16_4 : CN_F16_8;
    P.w2 = wf_w2_lds<FEAT>(L);
    const size_t geom = (FEAT & RTW_F_GEOM) ? L.geom_lds : 0u;  // quads / members / instances
    const size_t compact = (L.cnodes && L.fast_box && L.wf_clds)
                               ? (size_t)L.n_nodes * L.n_orders * (L.cnode32 ? 32u : 16u) : 0;
    const size_t need = (size_t)L.n_nodes * L.n_orders * 32u;
    const size_t nodes32 = (L.wf_lds && need <= RTW_WF_LDS_MAX) ? (need + 511u) / 512u * 512u : 0;
    const bool tail_staged = (L.wf_fuse & 2u) != 0;

    if ((FEAT & RTW_WF_NO_CLDS) == 0 && compact && compact + cur1 <= RTW_WF_CLDS_MAX) P.f_clds = compact;
    if (!P.f_clds) P.f_lds = nodes32;
    // The compact stage's block shape: the 8-copy stage (C2: 124 KB) leaves room for one 1024-thread block
    // per CU; the 4-copy stage (L.n_orders == 4, 62 KB) for two 768-thread blocks (rtw_tuning.clds_shape 4)
    // when it fits half the LDS
    P.two = P.f_clds && P.cn == CN_F16_4 && P.f_clds + cur2 <= RTW_WF_CLDS2_MAX && L.clds_shape == 4u;
    const size_t with_mats = P.f_clds + L.mat_lds + cur1 <= 160u * 1024u ? P.f_clds + L.mat_lds : P.f_clds;
    P.f_step_clds = P.two && with_mats + cur2 > RTW_WF_CLDS2_MAX ? P.f_clds : with_mats;  // only if they fit too
    P.f_step_lds = P.f_lds + (L.perlin_lds ? (size_t)L.n_perlin * RTW_PERLIN_BYTES : 0) + geom + L.shade_lds;
    P.f_tail_clds = tail_staged ? P.f_clds : 0;
    P.f_tail_lds = tail_staged && P.f_lds ? P.f_lds + geom + L.shade_lds : 0;
    // measured: fused wins on C2 (+8.5 %), C5 (+24 %), Cornell (+2 %) and, since the
    // round-3 queues and object trees, Cornell smoke (media: +23 %); through L1/L2 (C4, RTW_WF_FUSE
    // bit 2) it loses (-13 %)
    P.fused = (L.wf_fuse & 1u) && (P.f_clds || P.f_lds || (L.wf_fuse & 4u));

    // compact nodes of every octant copy in LDS (small static sphere trees, textured ones too)
    if ((FEAT & (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_MOVING)) == 0 && compact <= RTW_WF_CLDS_MAX) P.s_clds = compact;
    P.s_trace_lds = nodes32 ? nodes32 + geom : 0;
    P.s_tail_lds = tail_staged && nodes32 ? P.s_trace_lds + L.shade_lds : 0;  // (smoke +5 %)
    return P;
}

// The tail launch over iteration it's queue: on the compact stage (`clds` bytes), on the 32-B stage with the
// geometry and the materials (`lds` bytes), else through L1/L2.  The counted kernels (CNT 1) run on the grid of
// their CNT 0 instantiation.
template <uint32_t FEAT>
void wf_launch_tail(const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu, const WfStage& P, size_t clds,
                    size_t lds, uint32_t it) {
    if constexpr ((FEAT & RTW_WF_NO_CLDS) == 0) {
        if (clds && P.two) {
            const uint32_t grid = wf_grid_for(wf_tail_clds2<FEAT, 768, 0>, n_cu, clds, 768);
            wf_with_cnt(L, [&](auto cnt) { wf_launch(wf_tail_clds2<FEAT, 768, cnt>, grid, 768, clds, st, L, W, it); });
            return;
        }
        if (clds) {
            wf_with_cn(P.cn, [&](auto cn) {
                const uint32_t grid = wf_grid_for(wf_tail_clds<FEAT, cn>, n_cu, clds, 1024);
                wf_launch(wf_tail_clds<FEAT, cn>, grid, 1024, clds, st, L, W, it);
            });
            return;
        }
    }
    if (lds) {
        const uint32_t grid = wf_grid_for(wf_tail_lds<FEAT, 0>, n_cu, lds);
        wf_with_cnt(L, [&](auto cnt) { wf_launch(wf_tail_lds<FEAT, cnt>, grid, 256, lds, st, L, W, it); });
    } else if constexpr ((FEAT & ~RTW_F_CHECKER) == 0) {
        const uint32_t grid = wf_grid_for(wf_tail_w5<FEAT, 0>, n_cu, P.w2);
        wf_with_cnt(L, [&](auto cnt) { wf_launch(wf_tail_w5<FEAT, cnt>, grid, 256, P.w2, st, L, W, it); });
    } else {
        wf_launch(wf_tail<FEAT>, wf_grid_for(wf_tail<FEAT>, n_cu, P.w2), 256, P.w2, st, L, W, it);
    }
}

// Fused path: one wf_step* kernel per iteration, then the tail and the reduce.
template <uint32_t FEAT>
void wf_run_fused(const rtw_launch& L, const rtw_wf& W0, hipStream_t st, int n_cu, const WfStage& P, rtw_timer* T) {
    const size_t clds = P.f_clds, lds = P.f_lds, cdyn = P.f_step_clds;
    // The step's grid.  Every form of a step runs on the grid of one instantiation, whose occupancy is the one
    // queried: the counted kernels (CNT 1) on their CNT 0 kernel's, and the iteration-0 (IT0 1) and later-iteration
    // (IT0 0) kernels of wf_step<FEAT, true> and wf_step_clds2 on that of the IT0 2 instantiation (either
    // iteration), which nothing launches -- the stripes are sized from it (wf_class_waves).
    uint32_t grid = 0;
    if constexpr ((FEAT & RTW_WF_NO_CLDS) == 0) {
        if (clds && P.two) grid = wf_grid_for(wf_step_clds2<FEAT, 768, 0>, n_cu, cdyn, 768);
        else if (clds) wf_with_cn(P.cn, [&](auto cn) { grid = wf_grid_for(wf_step_clds<FEAT, cn>, n_cu, cdyn, 1024); });
    }
    if (!clds) grid = lds ? wf_grid_for(wf_step<FEAT, true, 0>, n_cu, P.f_step_lds)
                          : wf_grid_for(wf_step<FEAT, false, 0>, n_cu, P.w2);
    // iteration 0 appends to len[1]; every later iteration's output counters are
    // zeroed by the kernel two iterations before (wf_step_zero_next)
    (void)hipMemsetAsync(W0.len[1], 0, RTW_WF_STRIPES * RTW_WF_LEN_STRIDE * 4, st);
    if (W0.deal) (void)hipMemsetAsync(W0.deal, 0, RTW_WF_DEAL_COUNTERS * 4, st);
    rtw_wf W = wf_coherence(W0, grid * (clds ? (P.two ? 768u : 1024u) / 64u : 4u), W0.sort_iters);
    W.packed = wf_packed<FEAT>() ? 1u : 0u;  // the fused step and its tail: always the packed state
    const uint32_t iters = L.max_depth < W.iters ? L.max_depth : W.iters;
    rtw_wf Wt = W;  // the camera-ray lists serve the LDS-staged steps of static sphere scenes
    if ((clds || lds) && iters) Wt = wf_lists<FEAT>(L, W, st);
    else Wt.tl_count = nullptr;
    // rayColor(depth <= 0) = 0 (camera.zig:183-185): no iteration writes W.ls, which holds the
    // previous render's radiance, so the reduce must add zeros
    if (iters == 0) (void)hipMemsetAsync(W.ls, 0, (size_t)W.n_paths * sizeof(rtw_rgb), st);
    rtw_launch Lc = L;  // the compact step stages the materials only when they fit
    if (cdyn == clds) Lc.mat_lds = 0;
    for (uint32_t it = 0; it < iters; it++) {
        RTW_TIME_BEGIN(T, RTW_K_TRACE)
        Wt.deal = W.deal;  // (only iteration 0 deals from it: counters 0 .. 511)
        // deal bit 16: iteration it >= 1 claims its stripes' chunks from counters of its own
        Wt.deal_it = (W.deal && (W.deal_mode & 16u) && it) ? W.deal + RTW_WF_DEAL_COUNTERS0 + it * RTW_WF_STRIPES
                                                           : nullptr;
        if (clds) {
            if constexpr ((FEAT & RTW_WF_NO_CLDS) == 0) {
                if (P.two && L.counters) {
                    wf_launch(wf_step_clds2<FEAT, 768, 1>, grid, 768, cdyn, st, Lc, Wt, it);
                } else if (P.two) {
                    wf_with_it0(it, [&](auto it0) {
                        wf_launch(wf_step_clds2<FEAT, 768, 0, it0>, grid, 768, cdyn, st, Lc, Wt, it);
                    });
                } else {
                    wf_with_cn(P.cn, [&](auto cn) {
                        wf_launch(wf_step_clds<FEAT, cn>, grid, 1024, cdyn, st, Lc, Wt, it);
                    });
                }
            }
        } else if (lds && L.counters) {
            wf_launch(wf_step<FEAT, true, 1>, grid, 256, P.f_step_lds, st, L, Wt, it);
        } else if (lds) {
            wf_with_it0(it, [&](auto it0) {
                wf_launch(wf_step<FEAT, true, 0, it0>, grid, 256, P.f_step_lds, st, L, Wt, it);
            });
        } else {
            wf_with_cnt(L, [&](auto cnt) { wf_launch(wf_step<FEAT, false, cnt>, grid, 256, P.w2, st, L, W, it); });
        }
        RTW_TIME_END(T)
    }
    if (iters < L.max_depth) {
        RTW_TIME_BEGIN(T, RTW_K_TAIL)
        rtw_wf Wd = W;  // the tail's input claims: counter 512 (iteration 0 took 0 .. 511)
        if (W.deal) Wd.deal = W.deal + RTW_WF_DEAL_LAUNCH;
        wf_launch_tail<FEAT>(L, Wd, st, n_cu, P, P.f_tail_clds, P.f_tail_lds, iters);
        RTW_TIME_END(T)
    }
    RTW_TIME_BEGIN(T, RTW_K_REDUCE)
    wf_launch(wf_reduce, (W.n_pix + 255u) / 256u, 256, 0, st, L, W);
    RTW_TIME_END(T)
}

// Split path: per iteration a trace and a shade kernel, then the tail and the reduce.
template <uint32_t FEAT>
void wf_run_split(const rtw_launch& L, const rtw_wf& W0, hipStream_t st, int n_cu, const WfStage& P, rtw_timer* T) {
    // (the shade kernels' grids at no dynamic LDS, as wf_class_waves counts them)
    const uint32_t shade = wf_grid_for(wf_shade<FEAT>, n_cu), shade0 = wf_grid_for(wf_shade<FEAT, true>, n_cu);
    const size_t shade_lds = (FEAT & RTW_F_GEOM) ? L.geom_lds : 0u;
    rtw_wf W = wf_coherence(W0, shade * 4u, W0.sort_iters_split);  // the split kernels' queues
    W.packed = wf_packed<FEAT>() ? 1u : 0u;  // the split kernels (and their tail) use the packed state too
    // dynamic deal: iteration 0's trace deals from counters 0 .. 511, its shade from 512 .. 1023
    if (W0.deal) (void)hipMemsetAsync(W0.deal, 0, RTW_WF_DEAL_COUNTERS * 4, st);
    const uint32_t iters = L.max_depth < W.iters ? L.max_depth : W.iters;
    // iteration 0's trace and shade generate the camera rays themselves (wf_camera); with no
    // iteration (max_depth 0) nothing writes W.ls and the reduce must add zeros
    if (iters == 0) (void)hipMemsetAsync(W.ls, 0, (size_t)W.n_paths * sizeof(rtw_rgb), st);
    const rtw_wf Wl = iters ? wf_lists<FEAT>(L, W, st) : W;  // camera rays: iteration 0 of wf_trace (L1/L2)
    for (uint32_t it = 0; it < iters; it++) {
        RTW_TIME_BEGIN(T, RTW_K_TRACE)
        // deal bit 16: iteration it >= 1's trace and shade claim their stripes' chunks from counters of their own;
        // iteration 0's shade deals from its own launch counters
        rtw_wf Wt = W, Ws = W;
        if (W.deal && (W.deal_mode & 16u) && it) {
            Wt.deal_it = W.deal + RTW_WF_DEAL_COUNTERS0 + it * RTW_WF_STRIPES;
            Ws.deal_it = W.deal + RTW_WF_DEAL_SHADE + it * RTW_WF_STRIPES;
        }
        if (W.deal && it == 0) Ws.deal = W.deal + RTW_WF_DEAL_LAUNCH;
        wf_with_it0(it, [&](auto it0) {
            constexpr bool cam = it0 != 0;
            if constexpr ((FEAT & (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_MOVING)) == 0) {
                if (P.s_clds) {
                    // one 1024-thread block per CU shares the stage (256 / 512: slower); every node
                    // form on the grid of the default one's (the Y4 forms: the same registers)
                    const uint32_t grid = wf_grid_for(wf_trace_clds<FEAT, cam>, n_cu, P.s_clds, 1024);
                    wf_with_cn(P.cn, [&](auto cn) {
                        wf_launch(wf_trace_clds<FEAT, cam, cn>, grid, 1024, P.s_clds, st, L, Wt, it);
                    });
                    return;
                }
            }
            if (P.s_trace_lds) {
                const uint32_t grid = wf_grid_for(wf_trace<FEAT, true, cam>, n_cu, P.s_trace_lds);
                wf_launch(wf_trace<FEAT, true, cam>, grid, 256, P.s_trace_lds, st, L, Wt, it);
            } else {  // (the camera-ray lists serve this one alone)
                const uint32_t grid = wf_grid_for(wf_trace<FEAT, false, cam>, n_cu, P.w2);
                wf_launch(wf_trace<FEAT, false, cam>, grid, 256, P.w2, st, L, cam ? Wl : Wt, it);
            }
        });
        RTW_TIME_END(T)
        RTW_TIME_BEGIN(T, RTW_K_SHADE)
        if (it == 0) wf_launch(wf_shade<FEAT, true>, shade0, 256, shade_lds, st, L, Ws, it);
        else wf_launch(wf_shade<FEAT>, shade, 256, shade_lds, st, L, Ws, it);
        RTW_TIME_END(T)
    }
    if (iters < L.max_depth) {
        RTW_TIME_BEGIN(T, RTW_K_TAIL)
        rtw_wf Wd = W;  // the tail's input claims: counter 1024 (iteration 0's trace and shade took 0 .. 1023)
        if (W.deal) Wd.deal = W.deal + 2 * RTW_WF_DEAL_LAUNCH;
        wf_launch_tail<FEAT>(L, Wd, st, n_cu, P, 0, P.s_tail_lds, iters);
        RTW_TIME_END(T)
    }
    RTW_TIME_BEGIN(T, RTW_K_REDUCE)
    wf_launch(wf_reduce, (W.n_pix + 255u) / 256u, 256, 0, st, L, W);
    RTW_TIME_END(T)
}

template <uint32_t FEAT>
void wf_run(const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu, rtw_timer* T) {
    const WfStage P = wf_stage<FEAT>(L);
    if (P.fused) wf_run_fused<FEAT>(L, W, st, n_cu, P, T);
    else wf_run_split<FEAT>(L, W, st, n_cu, P, T);
}

// Waves of the largest grid of class FEAT that rtw_wavefront_max_waves counts.  It sizes the stripes, which the
// kernels do not bound-check, so it must bound the grid of every kernel that pushes survivors into them
// (wf_push / wf_push_bucketed): wf_shade, wf_step, wf_step_clds and wf_step_clds2.
//   wf_shade, both instantiations: launched on exactly these grids (wf_run_split).
//   wf_step_clds, wf_step_clds2: counted here at no dynamic LDS, and more LDS never admits more blocks; the node
//     forms of wf_step_clds differ in the walk alone (one 1024-thread block per CU either way).
//   wf_step (256 threads): not counted.  Its grid is that of an instantiation compiled for RTW_WPE_STEP waves per
//     SIMD (wf_run_fused: the IT0 2, CNT 0 one; 4 waves in profiles/isa_resources.json), below the RTW_WPE_SHADE
//     waves of the sphere classes' wf_shade -- the maximum is taken over every class of every unit, so those bound
//     the classes whose own wf_shade needs more registers than their wf_step.
static_assert(RTW_WPE_STEP <= RTW_WPE_SHADE, "the sphere classes' shade grids bound the fused step's (wf_class_waves)");
template <uint32_t FEAT>
uint32_t wf_class_waves(int n_cu) {
    uint32_t w = 4u * std::max(wf_grid_for(wf_shade<FEAT>, n_cu), wf_grid_for(wf_shade<FEAT, true>, n_cu));
    if constexpr ((FEAT & RTW_WF_NO_CLDS) == 0) {
        w = std::max({w, 12u * wf_grid_for(wf_step_clds2<FEAT, 768, 0>, n_cu, 0, 768),
                      16u * wf_grid_for(wf_step_clds<FEAT>, n_cu, 0, 1024)});
    }
    return w;
}

// Object scenes without media, image / noise textures or motion (quads, instances, lights,
// solid / checker textures: the Cornell box, HEAD's default scene) get their own
// instantiation: without the unused code paths the fused step needs fewer registers.
// Likewise static, unlit sphere scenes with image / noise textures (BASELINE config 5) and
// object scenes with media but no image / noise textures or motion (Cornell smoke).
#define RTW_F_OBJECTS (RTW_F_GEOM | RTW_F_LIGHT | RTW_F_CHECKER)
#define RTW_F_TEXTURED (RTW_F_CHECKER | RTW_F_IMAGE | RTW_F_NOISE)
#define RTW_F_MEDIA (RTW_F_GEOM | RTW_F_MEDIUM | RTW_F_LIGHT | RTW_F_CHECKER)
uint32_t wf_pick_feat(uint32_t f) {
    // registered vertex attributes or lights, instance trees: their own instantiations (rtw_internal.h)
    if (const uint32_t p = rtw_feat_prefix(f)) return p;
    if ((f & ~RTW_F_CHECKER) == 0) return f ? RTW_F_CHECKER : 0u;
    if ((f & RTW_F_GEOM) && (f & ~RTW_F_OBJECTS) == 0) return RTW_F_OBJECTS;
    if ((f & ~RTW_F_TEXTURED) == 0) return RTW_F_TEXTURED;
    if ((f & RTW_F_MEDIUM) && (f & ~RTW_F_MEDIA) == 0) return RTW_F_MEDIA;
    return (f & (RTW_F_GEOM | RTW_F_MEDIUM)) ? RTW_F_ALL : RTW_F_SPHERES;
}

// The classes (values of wf_pick_feat) whose kernels a translation unit instantiates, and what it exports of them
template <uint32_t... F>
struct WfClasses {
    // runs the batch if `feat` is one of them
    static bool run(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu, rtw_timer* T) {
        return ((feat == F && (wf_run<F>(L, W, st, n_cu, T), true)) || ...);
    }
    static uint32_t max_waves(int n_cu) { return std::max({wf_class_waves<F>(n_cu)...}); }
    // wf_lists_only of `feat` if it is one of them, else -1
    static int lists(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, uint32_t builder) {
        int r = -1;
        (void)((feat == F && (r = wf_lists_only<F>(L, W, st, builder), true)) || ...);
        return r;
    }
};

// The translation units, each with its class table:
//   WF_TU_SPHERES  untextured static sphere scenes (BASELINE C2, C3, C4; rtw_wavefront_spheres.hip), compiled with
//                  64-B loop alignment (csrc/Makefile): C2 +0.8 %, C3 +0.7 %; the other scene classes gained nothing
//                  from the flag (C5 -0.3 %, Cornell -0.4 %), so they keep the default placement
//   WF_TU_LIGHTS   contexts with registered lights (rtw_feat_of: RTW_F_PDF; rtw_wavefront_lights.hip)
//   WF_TU_ATTRS    contexts with registered vertex attributes (RTW_F_ATTR; rtw_wavefront_attrs.hip)
//   WF_TU_MAIN     every other class (rtw_wavefront.hip)
//   WF_TU_ENV      contexts with a registered environment (RTW_F_ENV; rtw_wavefront_env.hip)
enum { WF_TU_MAIN, WF_TU_SPHERES, WF_TU_LIGHTS, WF_TU_ATTRS, WF_TU_ENV };
#if defined(RTW_WF_ENV_TU)
constexpr int WF_TU = WF_TU_ENV;
using WfUnit = WfClasses<RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ENV,
                         RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR | RTW_F_ENV>;
#elif defined(RTW_WF_ATTRS_TU)
constexpr int WF_TU = WF_TU_ATTRS;
using WfUnit = WfClasses<RTW_F_ALL | RTW_F_TREE | RTW_F_ATTR, RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR>;
#elif defined(RTW_WF_LIGHTS_TU)
constexpr int WF_TU = WF_TU_LIGHTS;
using WfUnit = WfClasses<RTW_F_ALL | RTW_F_PDF, RTW_F_ALL | RTW_F_TREE | RTW_F_PDF>;
#elif defined(RTW_WF_SPHERES_TU)
constexpr int WF_TU = WF_TU_SPHERES;
using WfUnit = WfClasses<0u, RTW_F_CHECKER>;
#else
constexpr int WF_TU = WF_TU_MAIN;
using WfUnit = WfClasses<RTW_F_SPHERES, RTW_F_OBJECTS, RTW_F_TEXTURED, RTW_F_MEDIA, RTW_F_ALL, RTW_F_ALL | RTW_F_TREE>;
#endif

}  // namespace

// a unit's entry points: specialised in the unit itself, called from the main one
template <int TU>
bool rtw_wf_unit_run(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu, rtw_timer* T);
template <int TU>
uint32_t rtw_wf_unit_max_waves(int n_cu);
template <int TU>
int rtw_wf_unit_lists(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, uint32_t builder);
#define RTW_WF_UNIT(TU)                                                                                     \
    template <>                                                                                             \
    bool rtw_wf_unit_run<TU>(uint32_t, const rtw_launch&, const rtw_wf&, hipStream_t, int, rtw_timer*);     \
    template <>                                                                                             \
    uint32_t rtw_wf_unit_max_waves<TU>(int);                                                                \
    template <>                                                                                             \
    int rtw_wf_unit_lists<TU>(uint32_t, const rtw_launch&, const rtw_wf&, hipStream_t, uint32_t);
RTW_WF_UNIT(WF_TU_MAIN) RTW_WF_UNIT(WF_TU_SPHERES) RTW_WF_UNIT(WF_TU_LIGHTS) RTW_WF_UNIT(WF_TU_ATTRS) RTW_WF_UNIT(WF_TU_ENV)
#undef RTW_WF_UNIT

template <>
bool rtw_wf_unit_run<WF_TU>(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu,
                            rtw_timer* T) {
    return WfUnit::run(feat, L, W, st, n_cu, T);
}
template <>
uint32_t rtw_wf_unit_max_waves<WF_TU>(int n_cu) {
    return WfUnit::max_waves(n_cu);
}
template <>
int rtw_wf_unit_lists<WF_TU>(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, uint32_t builder) {
    return WfUnit::lists(feat, L, W, st, builder);
}

#if !defined(RTW_WF_ENV_TU) && !defined(RTW_WF_ATTRS_TU) && !defined(RTW_WF_LIGHTS_TU) && !defined(RTW_WF_SPHERES_TU)
template <int... TU>
struct WfUnits {
    static bool run(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, int n_cu, rtw_timer* T) {
        return (rtw_wf_unit_run<TU>(feat, L, W, st, n_cu, T) || ...);
    }
    static uint32_t max_waves(int n_cu) { return std::max({rtw_wf_unit_max_waves<TU>(n_cu)...}); }
    static bool lists(uint32_t feat, const rtw_launch& L, const rtw_wf& W, hipStream_t st, uint32_t builder) {
        int r = -1;
        (void)(((r = rtw_wf_unit_lists<TU>(feat, L, W, st, builder)) >= 0) || ...);
        return r > 0;
    }
};
using WfAllUnits = WfUnits<WF_TU_MAIN, WF_TU_SPHERES, WF_TU_LIGHTS, WF_TU_ATTRS, WF_TU_ENV>;

void rtw_wavefront_batch(const rtw_launch& L, const rtw_wf& W, void* stream, int n_cu, rtw_timer* T) {
    (void)WfAllUnits::run(wf_pick_feat(rtw_feat_of(L)), L, W, (hipStream_t)stream, n_cu, T);
}

uint32_t rtw_wavefront_max_waves(int n_cu) { return WfAllUnits::max_waves(n_cu); }

bool rtw_wavefront_tile_lists(const rtw_launch& L, const rtw_wf& W, void* stream, uint32_t builder) {
    return WfAllUnits::lists(wf_pick_feat(rtw_feat_of(L)), L, W, (hipStream_t)stream, builder);
}

// Host-only test hook (include/rtw_gpu.h): tile_frustum and tile_reach -- the list builders' code, the same fp32
// operations -- for the tile of pixels [x0, x1] x [y0, y1] and n spheres
extern "C" int rtw_debug_tile_reach(const rtw_camera* cam, float x0, float x1, float y0, float y1, uint32_t n,
                                    const float* centres, const float* radii, uint8_t* reach, float* tlow,
                                    uint8_t* frame_ok) {
    if (int rc = rtw_validate_cam(cam)) return rc;
    if (n && (!centres || !radii || !reach || !tlow)) {
        rtw_set_error("rtw_debug_tile_reach: null centres / radii / reach / tlow");
        return RTW_E_INVALID;
    }
    rtw_launch L{};
    rtw_launch_camera(L, cam, 0);
    const TileFrustum F = tile_frustum(L, x0, x1, y0, y1);
    if (frame_ok) *frame_ok = F.ok ? 1 : 0;
    for (uint32_t i = 0; i < n; i++) {
        float t = 0.0f;
        reach[i] = tile_reach(F, mk(centres[3 * (size_t)i], centres[3 * (size_t)i + 1], centres[3 * (size_t)i + 2]),
                              radii[i], t) ? 1 : 0;
        tlow[i] = t;
    }
    return RTW_OK;
}
#endif

#if defined(RTW_WF_SPHERES_TU) && defined(RTW_DIAG_WALK)
// (the sphere-scene kernels' records and counters: this translation unit's)
// diagnostic build only: where the per-slot walk records of iteration `it` go (null: off)
extern "C" int rtw_debug_walk_records(void* d_rec, uint32_t cap_slots, uint32_t it) {
    uint4* p = static_cast<uint4*>(d_rec);
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtw_diag_rec), &p, sizeof p) != hipSuccess) return RTW_E_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtw_diag_rec_cap), &cap_slots, 4) != hipSuccess) return RTW_E_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtw_diag_rec_it), &it, 4) != hipSuccess) return RTW_E_HIP;
    return RTW_OK;
}
// diagnostic build only: the compact walk's step counters (rtw_device.h WalkDiag), read and optionally reset
extern "C" int rtw_debug_walk_counters(uint64_t* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rtw_diag_walk), 16 * sizeof(uint64_t)) != hipSuccess) return RTW_E_HIP;
    if (reset) {
        const uint64_t z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(rtw_diag_walk), z, sizeof z) != hipSuccess) return RTW_E_HIP;
    }
    return RTW_OK;
}
#endif
