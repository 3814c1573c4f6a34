// db_gemm_body.inc -- the body of the many-query GEMM kernels of batch.hip, stated once and included by db_gemm_topk (PREFIX = false)
// and db_gemm_prefixed (PREFIX = true).  In scope where it is included: the template parameters KC, WN, KL, ROW; constexpr bool PREFIX;
// BatchArgs a; PrefixLimits lim (read only where PREFIX).  Included text rather than an inlined function: the listing of db_gemm_topk
// stays, instruction for instruction, what it was before the second kernel existed (profiles/query_prefix.md).
    constexpr bool CAST = std::is_same<ROW, double>::value;
    static_assert(CAST || std::is_same<ROW, float>::value, "float or double rows");
    static_assert(KC == 32, "one K-chunk = 8 slots of 4 floats per DB row");
    static_assert(WN == 2 || WN == 4, "tile 128 x 128 or 256 x 256");
    constexpr int TM = 64 * WN, TN = 64 * WN;            // tile: queries x DB rows
    constexpr int NT = 128 * WN, WAVES = 2 * WN;          // threads, waves
    constexpr int TILE = TM * KC;                         // floats of the A tile of one stage
    constexpr int BTILE = (TN / 8) * kBBlock;             // DB tile: TN / 8 blocks of 8 rows, kBBlock floats apart
    constexpr int STAGE = TILE + BTILE;                   // A tile then B tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *S0 = reinterpret_cast<float *>(smem);        // stage s: A = S0 + s*STAGE, B = A + TILE
    float *Ct = reinterpret_cast<float *>(smem);         // [TM][CT_LD] (aliases the stages after the K loop)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int D = a.D, K = a.K;
    const int q0 = blockIdx.y * TM;
    // DB tiles are handed out dynamically: workgroup x of a query tile starts on DB tile x and then takes the next unclaimed one
    // from a counter (one atomic per tile, ~1 ms of work; fetched at the start of the tile, read at its end).  With a static
    // split 3907 tiles over 256 workgroups cost 16 tile times on every CU; claimed tiles cost 15.26.  The lists a workgroup
    // keeps do not care which tiles fed them: the merged top-K is the same set whatever the assignment.
    __shared__ unsigned next_tile_slot;
    int64_t n_rows = a.n_rows;
    if constexpr (PREFIX) n_rows = lim.tile_limit[blockIdx.y];
    const int64_t n_tiles = (n_rows + TN - 1) / TN;

    // Top-k of the tile scores: ALL threads take part -- thread t owns query q0 + (t % TM) over the 64-column half (t / TM)
    // of every 128-column epilogue pass, with its sorted list in registers; the two lists of a query are folded at the end.
    // (Round 1 had 64 owner threads scan 2 x 128 columns while the other three waves -- and, in lockstep, the other workgroup
    // of the CU -- waited.)
    // (PREFIX: the column half is the wave's -- TM / 64 = WN waves per half -- and stays scalar; the epilogue and the fold read the lane
    // anew, so nothing of the thread's id lives in a register across the K loop on their account)
    const int oq = tid & (TM - 1), och = PREFIX ? wave / WN : tid / TM;
    TopList<KL> L;
    list_init(L);

    const int n_chunks = D / KC;
    // A loader: the chunk image is contiguous (TM * 128 B): pass u, wave w copies bytes [(u * WAVES + w) * 1024, + 1024)
    const float *const a_src = a.Qt + ((int64_t)blockIdx.y * n_chunks) * TILE + (wave * 64 + lane) * 4;
    const float *const a_tile = a.Qt + ((int64_t)blockIdx.y * n_chunks) * TILE;   // PREFIX: the same copy as scalar base + lane offset
    // B loader: pass u, wave w, lane i -> 8-row block u * WAVES + w, row i >> 3 of it, slot p = i & 7,
    // source floats [4 k4, 4 k4 + 4), k4 = p ^ (row & 7)
    const int l_row = wave * 8 + (lane >> 3), l_p = lane & 7;
    const int l_k4 = (l_p ^ (lane >> 3)) * 4;
    // fragment map
    const int fr = lane & 31, fk = lane >> 5;
    const int rb0 = wn * 64 + fr, rb1 = rb0 + 32;
    const int b_off0 = TILE + b_row_off(rb0) + fk, b_off1 = TILE + b_row_off(rb1) + fk, sw0 = rb0 & 7, sw1 = rb1 & 7;
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(S0));

    // Units of work: the first n_full = floor(n_tiles / P) * P tiles are whole tiles (P = workgroups of this query tile: full
    // rounds in which every CU is busy); what remains -- r < P tiles, the round that would leave P - r CUs idle -- is cut
    // into query halves when 2 r <= P (each wave then owns WN / 2 x 2 blocks and the unit takes half a tile time: 15.5 instead of
    // 16 tile times for 3907 tiles on 256 CUs).
    const int64_t n_full = n_tiles / gridDim.x * gridDim.x;
    const bool halves = 2 * (n_tiles - n_full) <= (int64_t)gridDim.x;
    const int64_t n_units = halves ? n_full + 2 * (n_tiles - n_full) : n_tiles;
    for (int64_t unit = blockIdx.x; unit < n_units;) {
        const bool half_unit = halves && unit >= n_full;
        const int64_t tile = half_unit ? n_full + ((unit - n_full) >> 1) : unit;
        const int qhalf = half_unit ? (int)((unit - n_full) & 1) : 0;
        const int nrb = half_unit ? WN / 2 : WN;                                      // 32-query row blocks per wave in this unit
        const int qrow0 = half_unit ? qhalf * (TM / 2) + wm * (16 * WN) : wm * (32 * WN);   // first query row of this wave
        const int a_off = fk * TM + qrow0 + fr;                        // + kk * 2 TM per k-step, + 32 i for row block i
        const int64_t n0 = tile * TN;
        unsigned claimed = 0;
        if (tid == 0) claimed = __hip_atomic_fetch_add(a.tile_ctr + blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (PREFIX) {
            if (tid == 0) (void)__hip_atomic_fetch_add(lim.done + blockIdx.y, half_unit ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const float *brow[4];
        // double rows: a tile lies within one segment (seg_rows is a multiple of TN: batch_local_enqueue), so its rows are a
        // workgroup-uniform base plus 32-bit byte offsets (segments are at most 1 GiB); rows past the end read the tile's first row
        const char *seg = nullptr;
        uint32_t boff[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t br = n0 + u * (8 * WAVES) + l_row;
            if constexpr (CAST || PREFIX) {   // (PREFIX, float rows: the same addressing feeds the LDS-DMA -- scalar base, 32-bit offsets)
                const int64_t brc = br < n_rows ? br : n0;
                boff[u] = (uint32_t)(((brc & a.seg_mask) * (int64_t)D + l_k4) * (int64_t)sizeof(ROW));
            } else {
                const int64_t brc = br < n_rows ? br : 0;   // rows past the end: any valid row (their columns are never scanned)
                brow[u] = reinterpret_cast<const float *const *>(a.seg_table)[brc >> a.seg_shift] + (brc & a.seg_mask) * (int64_t)D + l_k4;
            }
        }
        if constexpr (CAST || PREFIX) {
            const uint64_t sp = (uint64_t)reinterpret_cast<const char *const *>(a.seg_table)[n0 >> a.seg_shift];
            // (readfirstlane returns int: each half goes through uint32_t, or a low word with bit 31 set would sign-extend over the high one)
            const uint32_t sp_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sp >> 32)), sp_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sp);
            seg = (const char *)(((uint64_t)sp_hi << 32) | sp_lo);
        }
        f32x16 acc[WN][2];
#pragma unroll
        for (int i = 0; i < WN; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

        // chunk c -> stage c % NST: 8 LDS-DMA instructions per wave, number j = 2 u + (0: A, 1: B)
        auto stage_load_one = [&](int c, int j) {
            const uint32_t st = lds_base + (uint32_t)((c % NST) * STAGE) * 4u;
            const int u = j >> 1;
            if (j & 1) {
                if constexpr (!CAST && PREFIX) glds16_s(seg + c * (KC * 4), boff[u], st + (uint32_t)(TILE + b_row_off((u * WAVES + wave) * 8)) * 4u);
                else if constexpr (!CAST) glds16(brow[u] + c * KC, st + (uint32_t)(TILE + b_row_off((u * WAVES + wave) * 8)) * 4u);
            } else if constexpr (PREFIX) glds16_s(a_tile + (int64_t)c * TILE + u * (WAVES * 256), (uint32_t)(wave * 64 + lane) * 16u, st + (uint32_t)((u * WAVES + wave) * 256) * 4u);
            else glds16(a_src + (int64_t)c * TILE + u * (WAVES * 256), st + (uint32_t)((u * WAVES + wave) * 256) * 4u);
        };
        auto stage_load = [&](int c) {
#pragma unroll
            for (int j = 0; j < 8; j++) stage_load_one(c, j);
        };
        // double rows: slot u of chunk c through registers (the slots of a thread are lane-linear in block u * WAVES + wave)
        auto cast_load = [&](int c, int u, f64x2 *r) {
            if constexpr (CAST) {
                const auto *chunk = (const __attribute__((address_space(1))) char *)seg + (int64_t)c * (KC * 8);
                const auto *p = (const __attribute__((address_space(1))) f64x2 *)(chunk + boff[u]);
                r[0] = p[0];
                r[1] = p[1];
            }
        };
        auto cast_store = [&](int c, int u, const f64x2 *r) {
            if constexpr (CAST) {
                float *d = S0 + (c % NST) * STAGE + TILE + b_row_off((u * WAVES + wave) * 8) + lane * 4;
                const float x = (float)r[0][0], y = (float)r[0][1], z = (float)r[1][0], w = (float)r[1][1];
                if ((wave & 3) == 0) lds_store_slot<16>(d, x, y, z, w);
                else if ((wave & 3) == 2) lds_store_slot<8>(d, x, y, z, w);
                else lds_store_slot<4>(d, x, y, z, w);
            }
        };
        if (n_chunks > 0) {
            stage_load(0);
            if constexpr (CAST) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    f64x2 r[2];
                    cast_load(0, u, r);
                    cast_store(0, u, r);
                }
            }
        }
        wait_loads_and_barrier();   // chunk 0 has landed
        // the K loop, instantiated for whole tiles (NRB = WN row blocks per wave) and for query halves (NRB = WN / 2)
        auto k_loop = [&](auto nrb_tag) {
            constexpr int NRB = decltype(nrb_tag)::value;
            for (int c = 0; c < n_chunks; c++) {
                const float *St = S0 + (c % NST) * STAGE;
                // chunk c + 1 goes to the stage last read in iteration c-1 (barrier since).  When its 8 LDS-DMA instructions are
                // issued matters (a burst keeps a wave from issuing MFMAs for ~300 cycles; a late load is waited for at the barrier):
                //   128 tile  all 8 at once at the top (the other workgroup's wave fills the gap: 119.4 TF vs 114.8 spread);
                //   256 tile  two in front of each of MFMA groups 1..4 (both waves of a SIMD belong to this workgroup and burst
                //             together: 0.814 of peak vs 0.792 for the burst, 0.805 for groups 0..3, 0.76 for one per group).
                //   double rows, both tiles: a thread's four slots in two halves through 16 staging registers -- slots 0, 1 loaded in
                //             front of group 0 and stored in front of group 3, where slots 2, 3 are loaded, stored in front of group 7;
                //             the A-side DMA in front of groups 0 and 1 (a store waits for every load issued before it: all of them
                //             are two groups old by then).
                const bool prefetch = c + 1 < n_chunks;
                if (!CAST && WN == 2 && prefetch) stage_load(c + 1);
                f64x2 raw[2][2];
                // fragments of k-steps (2 k4, 2 k4 + 1) in f[k4 & 1]: [2 i + t] = A row block i, [2 WN + 2 j + t] = B block j;
                // the next pair is read before this pair's 4 WN MFMAs are issued
                float f[2][2 * WN + 4];
                auto rd = [&](int k4, float *d) {
#pragma unroll
                    for (int i = 0; i < NRB; i++) {
                        d[2 * i] = St[a_off + 32 * i + (2 * k4) * (2 * TM)];
                        d[2 * i + 1] = St[a_off + 32 * i + (2 * k4 + 1) * (2 * TM)];
                    }
                    const int p0 = (k4 ^ sw0) << 2, p1 = (k4 ^ sw1) << 2;
                    d[2 * WN] = St[b_off0 + p0];     d[2 * WN + 1] = St[b_off0 + p0 + 2];
                    d[2 * WN + 2] = St[b_off1 + p1]; d[2 * WN + 3] = St[b_off1 + p1 + 2];
                };
                rd(0, f[0]);
                __builtin_amdgcn_sched_group_barrier(0x100, NRB + 2, 0);  // the reads of the first pair
#pragma unroll
                for (int k4 = 0; k4 < KC / 4; k4++) {
                    if (!CAST && WN == 4 && prefetch && k4 >= 1 && k4 <= 4) { stage_load_one(c + 1, 2 * k4 - 2); stage_load_one(c + 1, 2 * k4 - 1); }
                    if (CAST && prefetch && k4 == 0) { cast_load(c + 1, 0, raw[0]); cast_load(c + 1, 1, raw[1]); }
                    if (CAST && prefetch && k4 <= 1) { stage_load_one(c + 1, 4 * k4); stage_load_one(c + 1, 4 * k4 + 2); }
                    if (CAST && prefetch && k4 == 3) {
                        cast_store(c + 1, 0, raw[0]); cast_store(c + 1, 1, raw[1]);
                        cast_load(c + 1, 2, raw[0]); cast_load(c + 1, 3, raw[1]);
                    }
                    if (CAST && prefetch && k4 == 7) { cast_store(c + 1, 2, raw[0]); cast_store(c + 1, 3, raw[1]); }
                    if (k4 + 1 < KC / 4) rd(k4 + 1, f[(k4 + 1) & 1]);
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const float b0 = f[k4 & 1][2 * WN + t], b1 = f[k4 & 1][2 * WN + 2 + t];
#pragma unroll
                        for (int i = 0; i < NRB; i++) {
                            const float av = f[k4 & 1][2 * i + t];
                            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[i][0], 0, 0, 0);
                            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[i][1], 0, 0, 0);
                        }
                    }
                    // keep the order "reads of the next pair, then this pair's MFMAs" through the scheduler
                    __builtin_amdgcn_sched_group_barrier(0x100, NRB + 2, 0);   // DS reads (ds_read2)
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NRB, 0);   // MFMA
                }
                // chunk c+1 has landed (no chunk behind it has been issued), every wave is done reading stage c % NST
                wait_loads_and_barrier();
            }
        };
        if (half_unit) k_loop(std::integral_constant<int, WN / 2>{});
        else k_loop(std::integral_constant<int, WN>{});
        // ---- epilogue: the score tile through LDS, 128 DB rows (two of the WN wave columns) per pass (the stages are free:
        // the K loop ended with a barrier); C/D layout of the MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
        const int ncols = (n_rows - n0) < TN ? (int)(n_rows - n0) : TN;
        // double rows: the epilogue's addresses are recomputed per tile from an opaque copy of the lane -- hoisted out of the tile loop
        // they would sit in registers the staging needs through the K loop (and spill)
        int elane = lane, eoq = oq;
        if constexpr (PREFIX) {
            elane = lane_now();
            eoq = (wave * 64 + elane) & (TM - 1);
        } else if constexpr (CAST) asm volatile("" : "+v"(elane), "+v"(eoq));
        // the query's own limit as columns of this tile (fetched per tile: an L2 hit, and no register held through the K loop)
        int64_t qcols = 0;
        if constexpr (PREFIX) qcols = (int64_t)lim.q_limit[q0 + eoq] - n0;
#pragma unroll
        for (int h = 0; h < WN / 2; h++) {
            if (h > 0) __syncthreads();   // the previous pass's scan is done with Ct
            if ((wn >> 1) == h) {
#pragma unroll
                for (int it = 0; it < WN; it++) {
                    if (it >= nrb) continue;   // a query half: the upper row blocks hold nothing
#pragma unroll
                    for (int jt = 0; jt < 2; jt++)
#pragma unroll
                        for (int e = 0; e < 16; e++) {
                            const int row = qrow0 + it * 32 + (e & 3) + 8 * (e >> 2) + 4 * (elane >> 5);   // query within the tile
                            const int col = (wn & 1) * 64 + jt * 32 + (elane & 31);                                  // DB row within the pass
                            Ct[row * CT_LD + col] = acc[it][jt][e];
                        }
                }
            }
            __syncthreads();
            float ts;
            int32_t tr;
            list_kth(L, K, ts, tr);
            const int pass_cols = ncols - h * 128;         // columns of this pass that exist
            const bool mine = !half_unit || (eoq >= qhalf * (TM / 2) && eoq < (qhalf + 1) * (TM / 2));   // a query half: only its queries have scores
            int c_hi = !mine ? 0 : pass_cols < (och + 1) * 64 ? pass_cols : (och + 1) * 64;
            if constexpr (PREFIX) {
                if (qcols - h * 128 < c_hi) c_hi = (int)(qcols - h * 128);   // (may be negative: nothing of this pass is the query's)
            }
            for (int c = och * 64; c < c_hi; c++) {
                const float s = Ct[eoq * CT_LD + c];
                const int32_t row = (int32_t)(n0 + h * 128 + c);
                if (fkey_gt(s, row, ts, tr)) {   // NaN never enters
                    list_push(L, K, s, row);
                    list_kth(L, K, ts, tr);
                }
            }
        }
        // next tile: published by thread 0, read by everyone after the barrier that also ends this tile's use of Ct
        if constexpr (PREFIX) {
            if (wave == 0 && elane == 0) next_tile_slot = gridDim.x + claimed;
        } else if (tid == 0) next_tile_slot = gridDim.x + claimed;
        __syncthreads();
        if constexpr (CAST || PREFIX) unit = __builtin_amdgcn_readfirstlane(next_tile_slot);   // (registers: the tile's bookkeeping stays scalar)
        else unit = next_tile_slot;
    }
    // fold the two column-half lists of a query into one (through LDS, once per workgroup): one list per (partition, query)
    __syncthreads();
    float *const Ls = reinterpret_cast<float *>(smem);                 // [TM][KL]
    int32_t *const Lr = reinterpret_cast<int32_t *>(Ls + TM * KL);
    int foq = oq;
    if constexpr (PREFIX) foq = (wave * 64 + lane_now()) & (TM - 1);
    if (och == 1) {
#pragma unroll
        for (int j = 0; j < KL; j++) { Ls[foq * KL + j] = L.s[j]; Lr[foq * KL + j] = L.r[j]; }
    }
    __syncthreads();
    if (och == 0) {
        for (int j = 0; j < K; j++) {
            const float s = Ls[foq * KL + j];
            const int32_t row = Lr[foq * KL + j];
            float ts;
            int32_t tr;
            list_kth(L, K, ts, tr);
            if (row >= 0 && fkey_gt(s, row, ts, tr)) list_push(L, K, s, row);
        }
        chip_topk_entry *dst = a.partial + ((int64_t)blockIdx.x * a.Qpad + q0 + foq) * K;
#pragma unroll
        for (int j = 0; j < KL; j++)
            if (j < K) {
                chip_topk_entry e;
                e.score = (double)L.s[j];
                e.idx = L.r[j] >= 0 ? (int64_t)L.r[j] * a.idx_mul + a.idx_add : -1;
                dst[j] = e;
            }
    }
    (void)NT;
