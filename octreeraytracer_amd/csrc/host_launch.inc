// Included by ort_kernel.hip after host_scene.inc.  The kernel dispatchers: a runtime choice of a
// kernel template's instance (pick), one launch_* per kernel family, and the persistent grids' sizes.
namespace {

// The dispatchers below stand in the order of their kernels in the code object (a kernel template
// is emitted where it is first named): moving one reorders the device code.
// A runtime int as a template argument: f(std::integral_constant<int, V>) for the first listed V
// equal to v, the LAST listed one when none is.  Every dispatcher below lists exactly the
// combinations it compiles: a kernel instance exists only where one of them names it.
template <int V, int... Rest, class F>
inline auto pick(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : pick<Rest...>(v, f);
}
#define ORT_V(x) decltype(x)::value  // the constant a pick() lambda was handed

// The shade kernel of a bounce: DIRECT, bounce 0 into a tight float tile (ort_render's own output),
// bounce 0 into any other output, a later bounce.
hipError_t launch_shade(int mode, bool first, bool direct, const PipeArgs& a, int blocks, hipStream_t s) {
    const dim3 g(blocks), t(kBlock);
    const bool tight_f32 = a.out_format == ORT_FORMAT_RGB32F && a.out_place == ORT_PLACE_TILE &&
                           a.out_pitch == 12u * (unsigned)a.tm.tw;
    pick<0, 1, 2>(mode, [&](auto MODE) {
        if (direct) hipLaunchKernelGGL((ort_shade_kernel<ORT_V(MODE), true, true>), g, t, 0, s, a);
        else if (first && tight_f32) hipLaunchKernelGGL((ort_shade_kernel<ORT_V(MODE), true, false>), g, t, 0, s, a);
        else if (first) hipLaunchKernelGGL((ort_shade_first_any<ORT_V(MODE)>), g, t, 0, s, a);
        else hipLaunchKernelGGL((ort_shade_kernel<ORT_V(MODE), false, false>), g, t, 0, s, a);
    });
    return hipGetLastError();
}

// Resident workgroups of a persistent grid (a plain launch: extra groups just start when others
// finish; no grid-wide synchronisation depends on residency), at most `needed`.
template <class K>
int resident_blocks(int device, K kernel, int threads, size_t lds, long long needed) {
    int per_cu = 0, cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    const long long b = (long long)std::max(per_cu, 1) * std::max(cus, 1);
    return (int)std::max(1LL, std::min(b, needed));
}

// ... of the persistent trace kernel
int persistent_blocks(int device, bool count, bool deep, int depth, size_t lds, long long needed) {
    const size_t dlds = lds_bytes(0, depth, false, kRevBounce, kPersistDeepBlock);
    return pick<1, 0>(count, [&](auto COUNT) {
        return deep ? resident_blocks(device, ort_trace_persistent<ORT_V(COUNT), true>, kPersistDeepBlock, dlds, needed)
                    : resident_blocks(device, ort_trace_persistent<ORT_V(COUNT), false>, kBlock, lds, needed);
    });
}

// One ort_pixel_paths launch (pm: 0 whole chains, 1 the samples' chunks in parallel, 2 recording or
// fixup; the variant of the scene's walk: brute force, a deep tree, an LDS-resident scene, or the
// plain compact walk) over a persistent grid sized by the variant's occupancy, at most `needed`
// workgroups.
hipError_t launch_pixel_paths(int pm, int device, int mode, bool deep, bool lds_scene, size_t lds, long long needed,
                              const PipeArgs& a, hipStream_t s) {
    const int variant = mode == 2 ? 0 : (deep ? 1 : (lds_scene ? 2 : 3));
    pick<2, 0, 1>(pm, [&](auto PM) {
        pick<0, 1, 2, 3>(variant, [&](auto V) {
            constexpr int MODE = ORT_V(V) == 0 ? 2 : 0;
            constexpr bool DEEP = ORT_V(V) == 1, LDS = ORT_V(V) == 2;
            const int g = resident_blocks(device, ort_pixel_paths<MODE, DEEP, LDS, ORT_V(PM)>, kBlock, lds, needed);
            hipLaunchKernelGGL((ort_pixel_paths<MODE, DEEP, LDS, ORT_V(PM)>), dim3(g), dim3(kBlock), lds, s, a);
        });
    });
    return hipGetLastError();
}

// The split walks of the listed heavy camera rays (FUSE 1: one bounce, shading fused; 2: bounce
// 0 of a longer path).
#ifndef ORT_SPLIT_BLOCKS
#define ORT_SPLIT_BLOCKS 32  // 1024 heavy rays in flight; more loop
#endif
hipError_t launch_trace_split(bool deep, int fmode, const PipeArgs& a, size_t lds, hipStream_t s) {
    pick<1, 0>(deep, [&](auto DEEP) {
        pick<1, 2>(fmode, [&](auto FUSE) {
            hipLaunchKernelGGL((ort_trace_split<ORT_V(DEEP) != 0, ORT_V(FUSE)>), dim3(ORT_SPLIT_BLOCKS), dim3(kBlock), lds, s, a);
        });
    });
    return hipGetLastError();
}

// The trace launch of a bounce: tile pairs, the persistent kernel over a list, the per-tile
// kernels of the compact layout, or the explicit-layout / brute-force kernel.
template <bool COUNT, bool PRIMARY>
hipError_t launch_trace_p(int mode, const PipeArgs& a, int blocks, int pblocks, size_t lds, hipStream_t s, int fuse) {
    const dim3 g(blocks), t(kBlock);
    const int deep = a.S.depth > 8;
    if (PRIMARY && mode == 0 && a.pair && pblocks == 0)  // tile pairs: blocks = workgroups (one per pair)
        pick<1, 0>(deep, [&](auto DEEP) {
            pick<1, 2, 0>(fuse, [&](auto FUSE) {
                if constexpr (ORT_V(DEEP)) hipLaunchKernelGGL((ort_trace_pair_deep<COUNT, ORT_V(FUSE)>), g, t, lds, s, a);
                else hipLaunchKernelGGL((ort_trace_pair<COUNT, ORT_V(FUSE)>), g, t, lds, s, a);
            });
        });
    else if (mode == 0 && pblocks > 0 && deep)
        hipLaunchKernelGGL((ort_trace_persistent<COUNT, true>), dim3(pblocks), dim3(kPersistDeepBlock),
                           lds_bytes(0, a.S.depth, false, kRevBounce, kPersistDeepBlock), s, a);
    else if (mode == 0 && pblocks > 0)
        hipLaunchKernelGGL((ort_trace_persistent<COUNT, false>), dim3(pblocks), t, lds, s, a);
    else if (mode == 0)
        pick<1, 0>(deep, [&](auto DEEP) {
            pick<1, 2, 0>(fuse, [&](auto FUSE) {
                if constexpr (ORT_V(DEEP)) hipLaunchKernelGGL((ort_trace_compact_deep<COUNT, PRIMARY, ORT_V(FUSE)>), g, t, lds, s, a);
                else hipLaunchKernelGGL((ort_trace_compact<COUNT, PRIMARY, ORT_V(FUSE)>), g, t, lds, s, a);
            });
        });
    else
        pick<1, 2>(mode, [&](auto MODE) { hipLaunchKernelGGL((ort_trace_kernel<ORT_V(MODE), COUNT, PRIMARY>), g, t, 0, s, a); });
    return hipGetLastError();
}

hipError_t launch_trace(bool count, int mode, bool primary, const PipeArgs& a, int blocks, int pblocks, size_t lds,
                        hipStream_t s, int fuse) {
    return pick<1, 0>(count, [&](auto COUNT) {
        return primary ? launch_trace_p<ORT_V(COUNT) != 0, true>(mode, a, blocks, pblocks, lds, s, fuse)
                       : launch_trace_p<ORT_V(COUNT) != 0, false>(mode, a, blocks, pblocks, lds, s, 0);
    });
}

// The exact walk of the deferred rays: a grid-stride loop over the (usually no) deferred rays; a
// small grid dispatches fast.  Seven instances: counting renders never fuse bounce 0 of a longer
// path (fmode 2), and only camera rays fuse at all.
hipError_t launch_trace_exact(bool count, bool prim, int fmode, const PipeArgs& a, size_t lds, hipStream_t s) {
    const dim3 g(256), t(kBlock);
    pick<1, 0>(count, [&](auto COUNT) {
        constexpr bool C = ORT_V(COUNT) != 0;
        if (fmode == 1) hipLaunchKernelGGL((ort_trace_exact<C, true, 1>), g, t, lds, s, a);
        else if (!C && fmode == 2) {
            if constexpr (!C) hipLaunchKernelGGL((ort_trace_exact<false, true, 2>), g, t, lds, s, a);
        } else if (prim) hipLaunchKernelGGL((ort_trace_exact<C, true, 0>), g, t, lds, s, a);
        else hipLaunchKernelGGL((ort_trace_exact<C, false, 0>), g, t, lds, s, a);
    });
    return hipGetLastError();
}

}  // namespace
