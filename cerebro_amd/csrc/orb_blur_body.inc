// orb_blur_body.inc -- the body of orb_blur (orb.hip), as text: included once by the single call's kernel, where ORB_FRAME(p, stride) is
// p and ORB_BLUR_LEVEL is blockIdx.z, and once by the batched put's fb_blur (blockIdx.z = level + n_levels * frame).  Text and not a
// __device__ function like the other stages: tests/test_codeobj_rectify.py pins the single kernel's registers, and an inlined function
// comes out of the compiler five vector registers apart from the kernel that states the same lines.  `a` is the OrbBlurArgs.
    __shared__ uint32_t tile[kBlurRows][kBlurDwords];
    __shared__ __align__(16) uint16_t hsum[kBlurRows][kBlurHPitch];
    const OrbBlurLevel &L = a.l[ORB_BLUR_LEVEL];
    const int tx0 = blockIdx.x * kBlurTileW, ty0 = blockIdx.y * kBlurTileH;
    if (tx0 >= L.bpitch || ty0 >= L.h) return;            // wave-uniform: the whole workgroup leaves (an empty level has h = 0)
    const uint8_t *img = ORB_FRAME(a.img, img_stride) + L.img_off;
    for (int i = threadIdx.x; i < kBlurRows * kBlurDwords; i += kOrbThreads) {
        const int r = i / kBlurDwords, cq = i - r * kBlurDwords;
        const int gy = min(max(ty0 - 3 + r, 0), L.h - 1);
        tile[r][cq] = orb_clamped_dword(img + (size_t)gy * L.pitch, tx0 - 4 + 4 * cq, L.w);
    }
    __syncthreads();
    // horizontal: four sums an item from three dwords (columns 4q - 4 .. 4q + 7 of the tile); 128 * 255 < 2^16
    for (int i = threadIdx.x; i < kBlurRows * (kBlurTileW / 4); i += kOrbThreads) {
        const int r = i / (kBlurTileW / 4), q = i - r * (kBlurTileW / 4);
        const uint32_t d0 = tile[r][q], d1 = tile[r][q + 1], d2 = tile[r][q + 2];
        uint32_t px[12];
#pragma unroll
        for (int b = 0; b < 4; b++) { px[b] = (d0 >> (8 * b)) & 255u; px[4 + b] = (d1 >> (8 * b)) & 255u; px[8 + b] = (d2 >> (8 * b)) & 255u; }
        uint32_t s[4];
#pragma unroll
        for (int k = 0; k < 4; k++)                       // pixel 4q + k is px[4 + k]
            s[k] = 9u * (px[1 + k] + px[7 + k]) + 17u * (px[2 + k] + px[6 + k]) + 24u * (px[3 + k] + px[5 + k]) + 28u * px[4 + k];
        *reinterpret_cast<uint2 *>(&hsum[r][4 * q]) = make_uint2(s[0] | s[1] << 16, s[2] | s[3] << 16);
    }
    __syncthreads();
    const int lx = threadIdx.x & 7, ly = threadIdx.x >> 3;
    const int x = tx0 + 16 * lx, y = ty0 + ly;
    if (x >= L.bpitch || y >= L.h) return;
    uint32_t acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 8192u;
    constexpr uint32_t g[7] = {9u, 17u, 24u, 28u, 24u, 17u, 9u};
#pragma unroll
    for (int j = 0; j < 7; j++) {
        const uint4 p = *reinterpret_cast<const uint4 *>(&hsum[ly + j][16 * lx]), q = *reinterpret_cast<const uint4 *>(&hsum[ly + j][16 * lx + 8]);
        const uint32_t d[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 8; k++) { acc[2 * k] += g[j] * (d[k] & 0xffffu); acc[2 * k + 1] += g[j] * (d[k] >> 16); }
    }
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        out[k] = (acc[4 * k] >> 14) | (acc[4 * k + 1] >> 14) << 8 | (acc[4 * k + 2] >> 14) << 16 | (acc[4 * k + 3] >> 14) << 24;
    *reinterpret_cast<uint4 *>(ORB_FRAME(a.blur, blur_stride) + L.blur_off + (size_t)y * L.bpitch + x) = make_uint4(out[0], out[1], out[2], out[3]);
