// The workgroup's part of a shape launch: the body of itx_shape_kernel and of inter_tb_shape_kernel (itx.hip), shared as TEXT.  It is
// not a device function on purpose: wrapping this body in a function, with nothing else changed, already alters the code the compiler
// makes for itx_shape_kernel (the function is optimised on its own before it is inlined), and the job-array kernels are to stay as they
// are.  The including kernel provides BD, LW, LH, PACKED and
//   default               jobs, n_jobs, lv...: a job array (host-built or written by itx_build_kernel); the residual is stored to job.coeffs
//                         and / or added to the rectangle at job.dst
//   ITX_SHAPE_RECORDS     src (InterTbSrc<BD>), n_jobs: jobs made in registers from vvc355_inter_tu records, residuals through InterEpi<BD>
    using px_t [[maybe_unused]] = typename Px<BD>::type;
    constexpr int W = 1 << LW, H = 1 << LH, CAP = W * H;
    constexpr int NT = CAP / 16, TBS = 256 / NT;             // lanes per block (one per 4x4 tile), blocks per workgroup
    using DV = TxDim<H>;                                     // vertical transform: k runs over rows
    using DH = TxDim<W>;                                     // horizontal transform: k runs over columns
    constexpr int KVV = DV::KV, PV = DV::P, KSV = DV::KS;
    constexpr int KVH = DH::KV, PH = DH::P, KSH = DH::KS;
    constexpr bool WAVE = NT <= 64;
    constexpr int CT_SZ = KVH * PV, TMP_SZ = H * PH;
    constexpr int FAST_BYTES = TBS * (CT_SZ + TMP_SZ) * 2, GEN_BYTES = CAP * 8;
    __shared__ __attribute__((aligned(16))) char lds_raw[FAST_BYTES > GEN_BYTES ? FAST_BYTES : GEN_BYTES];
    __shared__ __attribute__((aligned(16))) int16_t tab_v[DV::NTYPE * H * PV];
    __shared__ __attribute__((aligned(16))) int16_t tab_h_own[W == H ? 8 : DH::NTYPE * W * PH];
    __shared__ int8_t cos_lds[256];
    const int16_t *tab_h = W == H ? tab_v : tab_h_own;

    DV::stage(tab_v);
    if (W != H)
        DH::stage(tab_h_own);
    cos_lds[threadIdx.x] = d_tab_dct2_cos[threadIdx.x];

    const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
    const int wg = xcd_chunked(blockIdx.x, gridDim.x);
    const int ji = wg * TBS + sub;
#ifdef ITX_SHAPE_RECORDS
    vvc355_itx_job job;
    InterEpi<BD> epi;
    const bool valid = src.get(ji < n_jobs ? ji : n_jobs - 1, job, epi) && ji < n_jobs;       // a skipped record: not valid, harmless job
#else
    const bool valid = ji < n_jobs;
    vvc355_itx_job job = jobs[valid ? ji : n_jobs - 1];
    resolve_type(job);
#endif
    const int nzw = job.nzw, nzh = job.nzh, range = job.range, bd = job.bd ? job.bd : BD;
    const int trh = job.trh, trv = job.trv;
    const int sh_final = 5 + range - bd;
    bool ok = job.log2_w == LW && job.log2_h == LH && range <= 15 && sh_final >= 1 && trh < DH::NTYPE && trv < DV::NTYPE;
    const bool dc_only = W == H && trh == TX_DCT2 && trv == TX_DCT2 && nzw == 1 && nzh == 1;
    const int cntv = dc_only ? 1 : inputs_used(trv, H, nzh);                // rows the column pass reads
    const int cnt2 = inputs_used(trh, W, nzw);                              // columns the row pass reads
    ok &= cntv <= KVV && cnt2 <= KVH;
    const int cnt2r = (cnt2 + KSH - 1) & ~(KSH - 1);

    // this lane's tile for I/O and for the row pass
    const int y0 = (tid / (W / 4)) * 4, x0 = (tid % (W / 4)) * 4;
    int *coeffs = (int *)job.coeffs;
    const bool act = valid && ok;

    // prediction samples first: they are needed last
#ifdef ITX_SHAPE_RECORDS
    epi.prefetch(act, x0, y0);
#else
    uint8_t *dst = (uint8_t *)job.dst;
    uint2 praw[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        praw[r] = make_uint2(0, 0);
        if (act && dst) {
            const uint8_t *p = dst + row_off(y0 + r, job.dst_stride) + x0 * (int)sizeof(px_t);
            if (BD > 8) praw[r] = gld<uint2>(p);
            else praw[r].x = gld<uint32_t>(p);
        }
    }
#endif
    int c[4][4];
    const Dequant dq = itx_job_dequant(job, bd);
    const bool need = act && y0 < cntv && x0 < nzw && x0 < KVH;
    unsigned mag = 0;
    bool packed = false;
    uint4 pk[2];
    if constexpr (PACKED) {
#ifdef ITX_SHAPE_RECORDS
        const LvSrc ls = { nullptr, src.stream() };
        const vvc355_tb_levels lvr = src.levels_of(ji < n_jobs ? ji : n_jobs - 1);
#else
        const LvSrc ls = lv_src(lv...);
        const vvc355_tb_levels lvr = ls.lv[valid ? ji : n_jobs - 1];
#endif
        packed = !(lvr.flags & VVC355_LEVELS_INT32);
        const int16_t *g = packed && need ? lv_group(lvr, ls.levels, LW, x0, y0) : nullptr;
        pk[0] = pk[1] = make_uint4(0, 0, 0, 0);
        if (g) {
            pk[0] = gld<uint4>(g);
            pk[1] = gld<uint4>(g + 8);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int4 v = make_int4(0, 0, 0, 0);
        if (PACKED && packed) {
            if (y0 + r < cntv)
                v = unpack_i16x4(r & 1 ? make_uint2(pk[r >> 1].z, pk[r >> 1].w) : make_uint2(pk[r >> 1].x, pk[r >> 1].y));
        } else if (need && y0 + r < cntv) {
            v = gld<int4>(coeffs + (y0 + r) * W + x0);
        }
        if (dq.on) {
            const unsigned lv = (unsigned)(v.x ^ (v.x >> 31)) | (unsigned)(v.y ^ (v.y >> 31)) | (unsigned)(v.z ^ (v.z >> 31)) | (unsigned)(v.w ^ (v.w >> 31));
            if ((lv >> 15) == 0) {
                v.x = dq.apply_small(v.x, x0, y0 + r); v.y = dq.apply_small(v.y, x0 + 1, y0 + r);
                v.z = dq.apply_small(v.z, x0 + 2, y0 + r); v.w = dq.apply_small(v.w, x0 + 3, y0 + r);
            } else {
                v.x = dq.apply(v.x, x0, y0 + r); v.y = dq.apply(v.y, x0 + 1, y0 + r);
                v.z = dq.apply(v.z, x0 + 2, y0 + r); v.w = dq.apply(v.w, x0 + 3, y0 + r);
            }
        }
        c[r][0] = x0 + 0 < nzw ? v.x : 0; c[r][1] = x0 + 1 < nzw ? v.y : 0;
        c[r][2] = x0 + 2 < nzw ? v.z : 0; c[r][3] = x0 + 3 < nzw ? v.w : 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            mag |= (unsigned)(c[r][q] ^ (c[r][q] >> 31));
    }
    ok &= (mag >> 15) == 0;
    if (!__syncthreads_and(!valid || ok)) {
        // some block of this workgroup needs the generic arithmetic: redo them all, one after the other, 256 lanes each
        int *gbuf = (int *)lds_raw, *gtmp = gbuf + CAP;
        for (int b = 0; b < TBS; b++) {
            const int jb = wg * TBS + b;
            if (jb >= n_jobs)
                break;
#ifdef ITX_SHAPE_RECORDS
            vvc355_itx_job jg;
            InterEpi<BD> eg;
            if (src.get(jb, jg, eg)) {
                const vvc355_tb_levels r = src.levels_of(jb);
                itx_generic_block<BD, 256, CAP, true, false, InterEpi<BD>>(jg, gbuf, gtmp, cos_lds, threadIdx.x, &r, src.stream(), 0, 0, &eg);
            }
#else
            vvc355_itx_job jg = jobs[jb];
            resolve_type(jg);
            if (jg.log2_w + jg.log2_h <= LW + LH) {
                if constexpr (PACKED) {
                    const LvSrc ls = lv_src(lv...);
                    const vvc355_tb_levels r = ls.lv[jb];
                    itx_generic_block<BD, 256, CAP, true>(jg, gbuf, gtmp, cos_lds, threadIdx.x, &r, ls.levels);
                } else
                    itx_generic_block<BD, 256, CAP>(jg, gbuf, gtmp, cos_lds, threadIdx.x);
            }
#endif
            __syncthreads();
        }
        return;
    }
    if (WAVE && !valid)
        return;                                              // whole groups inside a wave; no workgroup barrier follows

    int16_t *cT = (int16_t *)lds_raw + sub * (CT_SZ + TMP_SZ), *tmp = cT + CT_SZ;
    if (y0 < KVV && x0 < KVH) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            *(uint2 *)&cT[(x0 + q) * PV + y0] = make_uint2(pack16(c[0][q], c[1][q]), pack16(c[2][q], c[3][q]));
    }
    group_sync<NT>();

    // ---- column pass: tile (rows ya.., columns xa..) of tmp, only the columns the row pass reads
    {
        constexpr int YT = H / 4;
        const int xa = (tid / YT) * 4, ya = (tid % YT) * 4;
        if (xa < cnt2r) {
            int acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[r][q] = 0;
            if (xa < nzw) {
                const int16_t *mrow = tab_v + (trv * H + ya) * PV;
                const int16_t *crow = cT + xa * PV;
                for (int k = 0; k < cntv; k += KSV) {
                    uint32_t m[4][KSV / 2], d[4][KSV / 2];
#pragma unroll
                    for (int r = 0; r < 4; r++) lds_row<KSV>(mrow + r * PV + k, m[r]);
#pragma unroll
                    for (int q = 0; q < 4; q++) lds_row<KSV>(crow + q * PV + k, d[q]);
#pragma unroll
                    for (int r = 0; r < 4; r++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
#pragma unroll
                            for (int e = 0; e < KSV / 2; e++) acc[r][q] = dot2(m[r][e], d[q][e], acc[r][q]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = clip_intp2((acc[r][q] + 64) >> 7, range);
                *(uint2 *)&tmp[(ya + r) * PH + xa] = make_uint2(pack16(v[0], v[1]), pack16(v[2], v[3]));
            }
        }
    }
    group_sync<NT>();

    // ---- row pass on this lane's I/O tile
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[r][q] = 0;
    {
        const int16_t *mrow = tab_h + (trh * W + x0) * PH;
        const int16_t *trow = tmp + y0 * PH;
        for (int k = 0; k < cnt2; k += KSH) {
            uint32_t m[4][KSH / 2], d[4][KSH / 2];
#pragma unroll
            for (int q = 0; q < 4; q++) lds_row<KSH>(mrow + q * PH + k, m[q]);
#pragma unroll
            for (int r = 0; r < 4; r++) lds_row<KSH>(trow + r * PH + k, d[r]);
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int e = 0; e < KSH / 2; e++) acc[r][q] = dot2(m[q][e], d[r][e], acc[r][q]);
        }
    }
    if (!valid)
        return;
    const int rnd = 1 << (sh_final - 1);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int res[4];
#pragma unroll
        for (int q = 0; q < 4; q++) res[q] = (acc[r][q] + rnd) >> sh_final;
#ifdef ITX_SHAPE_RECORDS
        epi.template row<W>(r, x0, y0 + r, res);
#else
        if (job.store_coeffs)
            gst<int4>(coeffs + (y0 + r) * W + x0, make_int4(res[0], res[1], res[2], res[3]));
        if (dst) {
            uint8_t *p = dst + row_off(y0 + r, job.dst_stride) + x0 * (int)sizeof(px_t);
            if (BD > 8) {
                const int o0 = clip_px<BD>((int)(praw[r].x & 0xffff) + res[0]), o1 = clip_px<BD>((int)(praw[r].x >> 16) + res[1]);
                const int o2 = clip_px<BD>((int)(praw[r].y & 0xffff) + res[2]), o3 = clip_px<BD>((int)(praw[r].y >> 16) + res[3]);
                gst<uint2>(p, make_uint2((uint32_t)o0 | ((uint32_t)o1 << 16), (uint32_t)o2 | ((uint32_t)o3 << 16)));
            } else {
                const uint32_t pr = praw[r].x;
                const int o0 = clip_px<BD>((int)(pr & 0xff) + res[0]), o1 = clip_px<BD>((int)((pr >> 8) & 0xff) + res[1]);
                const int o2 = clip_px<BD>((int)((pr >> 16) & 0xff) + res[2]), o3 = clip_px<BD>((int)(pr >> 24) + res[3]);
                gst<uint32_t>(p, (uint32_t)o0 | ((uint32_t)o1 << 8) | ((uint32_t)o2 << 16) | ((uint32_t)o3 << 24));
            }
        }
#endif
    }
