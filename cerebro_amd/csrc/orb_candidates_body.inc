// orb_candidates_body.inc -- the body of orb_candidates (orb.hip), as text: included once by the single call's kernel, where
// ORB_FRAME(p, which) is p, and once by the batched put's fb_candidates, where it is p + frame * stride.  Text and not a __device__
// function like the other stages: tests/test_codeobj_orb_describe.py and test_codeobj_rectify.py pin the single kernel's SGPR count, and
// an inlined function comes out of the compiler two scalar registers apart from the kernel that states the same lines.  `a` is the OrbArgs.
    __shared__ int32_t list[kStripMaxCand];
    __shared__ int32_t wave_n[kOrbThreads / 64];
    const OrbLevel &L = a.t.l[blockIdx.y];
    const int strip = blockIdx.x;
    if (strip >= L.nstrips) return;
    const int16_t *sc = ORB_FRAME(a.score, score) + L.score_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int thr = a.t.threshold;
    int base = 0;                                         // survivors so far, the same in every thread
    for (int r = 0; r < kStripRows; r++) {
        const int y = L.y0 + kStripRows * strip + r;
        if (y > L.y1) break;
        for (int xc = L.x0; xc <= L.x1; xc += kOrbThreads) {
            const int x = xc + (int)threadIdx.x;
            bool keep = false;
            if (x <= L.x1) {
                const int16_t *p = sc + (size_t)y * L.spitch + x;
                const int s = p[0];
                if (s >= thr) {
                    const int16_t *u = p - L.spitch, *d = p + L.spitch;
                    const int m = max(max(max((int)u[-1], (int)u[0]), max((int)u[1], (int)p[-1])), max(max((int)p[1], (int)d[-1]), max((int)d[0], (int)d[1])));
                    keep = s > m;
                }
            }
            const unsigned long long votes = __ballot(keep);
            if (lane == 0) wave_n[wave] = __popcll(votes);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kOrbThreads / 64; w++) { const int n = wave_n[w]; total += n; if (w < wave) before += n; }
            if (keep) {
                const int at = base + before + __popcll(votes & ((1ull << lane) - 1ull));
                if (at < L.cap) list[at] = y * L.w + x;  // (always: one strict maximum per 2 x 2 block; filled to cap by tests/test_orb_limits_gpu.py)
            }
            base += total;
            __syncthreads();
        }
    }
    const int n = min(base, L.cap);
    OrbCand *seg = ORB_FRAME(a.cand, cand) + L.cand_off + (size_t)strip * L.cap;
    const uint8_t *img = ORB_FRAME(a.img, img) + L.img_off;
    for (int i = threadIdx.x; i < n; i += kOrbThreads) {
        const int raster = list[i], y = raster / L.w, x = raster - y * L.w;
        const long long R = orb_harris(img, L.pitch, x, y);
        *reinterpret_cast<uint4 *>(seg + i) = make_uint4((uint32_t)(unsigned long long)R, (uint32_t)((unsigned long long)R >> 32), (uint32_t)raster, 0u);
    }
    if (threadIdx.x == 0) ORB_FRAME(a.strip_count, strip)[L.strip_off + strip] = n;
