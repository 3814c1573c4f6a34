// rectify_pair_body.inc -- the body of rectify_pair (frames.hip), as text: included once by the single call's kernel, where RECT_EYE is
// blockIdx.z and RECT_FRAME(p) is p, and once by the batched put's fb_rectify (blockIdx.z = eye + 2 * frame, RECT_FRAME(p) the frame's
// bytes behind p, a multiple of 16).  Text and not a __device__ function like the other stages of frames.hip: tests/test_project_codeobj.py
// pins the single kernel's registers, and an inlined function comes out of the compiler three vector registers apart from the kernel
// that states the same lines.  `g` is the RectifyArgs.
    const int x0 = kRectPix * (int)(blockIdx.x * kRectLanes + (threadIdx.x & (kRectLanes - 1)));
    const int y = (int)(blockIdx.y * kRectRows + threadIdx.x / kRectLanes);
    if (x0 >= g.w || y >= g.h) return;
    const size_t px = (size_t)g.w * g.h, eye = RECT_EYE;
    const uint8_t *raw = RECT_FRAME(g.raw) + eye * px;
    const int2 *q1 = g.q + eye * (size_t)g.stages * px, *q2 = q1 + px;
    const size_t row = (size_t)y * g.w;
    uint32_t out[kRectPix];
#pragma unroll
    for (int k = 0; k < kRectPix; k++) {
        const int x = min(x0 + k, g.w - 1);                               // a tail repeats the row's last pixel and stores nothing of it
        if (g.stages == 1) {
            const int2 m = q1[row + x];
            out[k] = (uint32_t)rect_sample(raw, g.w, g.h, m.x, m.y);
            continue;
        }
        const int2 m = q2[row + x];
        const int tx = m.x >> 5, a = m.x & 31, ty = m.y >> 5, b = m.y & 31;
        int u[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int ux = tx + (t & 1), uy = ty + (t >> 1);
            u[t] = 0;
            if ((unsigned)ux < (unsigned)g.w && (unsigned)uy < (unsigned)g.h) {
                const int2 m1 = q1[(size_t)uy * g.w + ux];
                u[t] = rect_sample(raw, g.w, g.h, m1.x, m1.y);
            }
        }
        out[k] = (uint32_t)((u[0] * (32 - a) * (32 - b) + u[1] * a * (32 - b) + u[2] * (32 - a) * b + u[3] * a * b + 512) >> 10);
    }
    const size_t o = eye * px + row + (size_t)x0;                         // g.out is aligned: the offset decides
    if (x0 + kRectPix <= g.w && (o & 3) == 0) {
        *reinterpret_cast<uint32_t *>(RECT_FRAME(g.out) + o) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
        return;
    }
    for (int k = 0; k < kRectPix && x0 + k < g.w; k++) RECT_FRAME(g.out)[o + k] = (uint8_t)out[k];
