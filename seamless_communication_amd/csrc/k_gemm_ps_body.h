// Body of the pre-split product kernels of k_gemm_ps.hip (the schedule is described there).  NOT a stand-alone header: it is
// included inside the braces of gemm_ps_kernel and of gemm_score_kernel, which supply
//   template / constexpr parameters  BM, BN, WGM, WGN, SPLIT, CONV, AMAX, SCORE, CAND, GLU
//   arguments                        GemmPsArgs p, tiles_n, tiles_total, tiles_per_xcd, a_bytes, w_bytes, GemmScoreArgs sc,
//                                    GemmCandArgs cd
// so that the kernels share every instruction of the K loop while gemm_ps_kernel keeps its own argument list.
// CAND (with SCORE; gemm_cand_kernel only): no target column; the wave also writes its value at every candidate column of
// cd.cand that lies in its column range.  Every statement of it sits behind `if constexpr (CAND)`.
// OOB and the vector types are device_util.h's, which k_gemm_ps.hip includes (this text sits inside a function body).
    constexpr int NWAVE = WGM * WGN;
    constexpr bool ALTERNATE = SPLIT && NWAVE == 8;  // the K loop's schedule, see above
    constexpr bool MID_BARRIER = SPLIT && !ALTERNATE;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int ACH = BM / (16 * NWAVE);  // 1 KB chunks (16 rows) of the A tile per wave
    constexpr int BCH = BN / (16 * NWAVE);
    constexpr int A_TILE = BM * 32, B_TILE = BN * 32;  // halfs per stage

    // three stages of [A_hi | A_lo | W] tiles (without SPLIT: [A_hi | W] - no LDS is set aside for a plane nobody stages: the
    // 128 x 128 tile then takes 48 KB instead of 72 and a CU holds three workgroups instead of two); after the K loop the same
    // memory holds one fp32 tile per wave for the transposed (row-major, 16 bytes per lane) epilogue
    constexpr int A_PL = SPLIT ? 2 : 1;
    constexpr int STAGE_BYTES = (A_PL * A_TILE + B_TILE) * 2;
    // columns of a wave's tile that go through LDS per epilogue pass: 64 where the stage memory holds such tiles, else 32
    constexpr int EPN = WN < 64 ? WN : (NWAVE * WM * (64 + 4) * 4 <= 3 * STAGE_BYTES ? 64 : 32);
    constexpr int EP_LD = EPN + 4;          // floats per row of a wave's epilogue tile
    static_assert(NWAVE * WM * EP_LD * 4 <= 3 * STAGE_BYTES, "epilogue tiles must fit in the stage memory");
    __shared__ __attribute__((aligned(16))) char smem[3 * STAGE_BYTES];
    _Float16* const sAh0 = reinterpret_cast<_Float16*>(smem);
    _Float16* const sAl0 = sAh0 + (A_PL - 1) * A_TILE;  // = sAh0 without SPLIT (never used then)
    _Float16* const sB0 = sAh0 + A_PL * A_TILE;
    _Float16* const sAh1 = reinterpret_cast<_Float16*>(smem + STAGE_BYTES);
    _Float16* const sAl1 = sAh1 + (A_PL - 1) * A_TILE;
    _Float16* const sB1 = sAh1 + A_PL * A_TILE;
    _Float16* const sAh2 = reinterpret_cast<_Float16*>(smem + 2 * STAGE_BYTES);
    _Float16* const sAl2 = sAh2 + (A_PL - 1) * A_TILE;
    _Float16* const sB2 = sAh2 + A_PL * A_TILE;

    const int bid = blockIdx.x;
    const int tile = (bid & 7) * tiles_per_xcd + (bid >> 3);
    if (tile >= tiles_total) return;
    const int tm = tile / tiles_n;
    const int tn = tile - tm * tiles_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = tm * BM, n0 = tn * BN;

    const i32x4_t rah = make_rsrc_words(p.Ah, a_bytes);
    const i32x4_t ral = make_rsrc_words(p.Al, a_bytes);
    const i32x4_t rw = make_rsrc_words(p.W, w_bytes);

    // this lane's fixed LDS position inside a chunk: row (lane >> 2), segment slot (lane & 3); it fetches the
    // global segment that the swizzle maps to that slot
    uint32_t a_voff[ACH], b_voff[BCH];
    int a_t[ACH];    // CONV: position of the lane's row inside its item
    int a_len[ACH];  // CONV: length of that item (rows_per_item, or row_pos[row].y for packed items)
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
        const int row = 16 * (wave * ACH + j) + (lane >> 2);
        const int seg = (lane & 3) ^ ((row >> 2) & 3);
        a_voff[j] = (m0 + row) < p.M ? (uint32_t)(((int64_t)(m0 + row) * p.lda + seg * 8) * 2) : OOB;
        a_t[j] = 0;
        a_len[j] = 0;
        if (CONV) {
            if (p.row_pos) {
                const int2 rp = (m0 + row) < p.M ? p.row_pos[m0 + row] : make_int2(0, 0);
                a_t[j] = rp.x;
                a_len[j] = rp.y;
            } else {
                a_t[j] = (m0 + row) % p.rows_per_item;
                a_len[j] = p.rows_per_item;
            }
        }
    }
    // CONV: (tap, 32-wide channel slab) of the NEXT slab to be issued - slabs are issued strictly in K order - and the
    // operand addresses of that slab: K byte offset inside the row (ka_) and row offset per chunk (va_), rows of another
    // item or outside the matrix as out-of-range offsets (hardware zero fill = the convolution's zero padding)
    int nx_tap = 0, nx_cs = 0, nx_slab = 0;
    const int spt = CONV ? p.conv_cin / PBK : 1;
    const uint32_t row_bytes = (uint32_t)(p.lda * 2);
    uint32_t va_[ACH];
    int ka_ = 0;
#define PS_NEXT_ADDR()                                                                                  \
    do {                                                                                                \
        if (CONV) {                                                                                     \
            const int dt_ = nx_tap * p.conv_dil - p.conv_pad;                                           \
            ka_ = nx_cs * (PBK * 2);                                                                    \
            _Pragma("unroll") for (int j = 0; j < ACH; ++j) {                                           \
                const bool in_ = (uint32_t)(a_t[j] + dt_) < (uint32_t)a_len[j] && a_voff[j] != OOB;     \
                va_[j] = in_ ? a_voff[j] + (uint32_t)dt_ * row_bytes : OOB;                             \
            }                                                                                           \
            if (++nx_cs == spt) {                                                                       \
                nx_cs = 0;                                                                              \
                ++nx_tap;                                                                               \
            }                                                                                           \
        } else {                                                                                        \
            ka_ = nx_slab * (PBK * 2);                                                                  \
            _Pragma("unroll") for (int j = 0; j < ACH; ++j) va_[j] = a_voff[j];                         \
        }                                                                                               \
        ++nx_slab;                                                                                      \
    } while (0)
#pragma unroll
    for (int j = 0; j < BCH; ++j) {
        const int row = 16 * (wave * BCH + j) + (lane >> 2);
        const int seg = (lane & 3) ^ ((row >> 2) & 3);
        b_voff[j] = (n0 + row) < p.N ? (uint32_t)(((int64_t)(n0 + row) * p.ldw + seg * 8) * 2) : OOB;
    }

    float16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets (bytes) per 16-wide K chunk kc = 0, 1
    int a_off[TM][2], b_off[TN][2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
        const int s = kc * 2 + (lane >> 5);
#pragma unroll
        for (int i = 0; i < TM; ++i) a_off[i][kc] = swz(wm * WM + i * 32 + (lane & 31), s);
#pragma unroll
        for (int j = 0; j < TN; ++j) b_off[j][kc] = swz(wn * WN + j * 32 + (lane & 31), s);
    }

// One LDS-DMA instruction: M0 = LDS byte address of this wave's 1 KB chunk, lane p lands at +16 p.  Issued as
// inline asm on purpose: the compiler cannot tell which LDS stage an in-flight DMA targets and would drain
// every outstanding DMA (s_waitcnt vmcnt(0)) before each ds_read; completion is awaited explicitly in PS_STEP.
#define PS_DMA(RSRC, LDSP, VOFF, SOFF)                                                                        \
    asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"                              \
                 :                                                                                            \
                 : "s"(__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)SC_LDS_PTR(LDSP))), "v"(VOFF), \
                   "s"(RSRC), "s"((int)(SOFF))                                                                \
                 : "memory")
#define PS_ISSUE(AH, AL, BB, KOFF)                                                             \
    do {                                                                                       \
        PS_NEXT_ADDR();                                                                        \
        _Pragma("unroll") for (int j = 0; j < ACH; ++j) {                                      \
            PS_DMA(rah, &AH[(wave * ACH + j) * 512], va_[j], ka_);                             \
            if (SPLIT) PS_DMA(ral, &AL[(wave * ACH + j) * 512], va_[j], ka_);                  \
        }                                                                                      \
        _Pragma("unroll") for (int j = 0; j < BCH; ++j)                                        \
            PS_DMA(rw, &BB[(wave * BCH + j) * 512], b_voff[j], (KOFF));                        \
    } while (0)

    constexpr int NDMA = 2 * ACH + BCH;                   // DMA slots per wave and slab (the lo slots stay empty without SPLIT)
    constexpr int NLIVE = SPLIT ? NDMA : ACH + BCH;       // DMA instructions really issued per wave and slab
    static_assert(NDMA == 6 || NDMA == 3, "two or one 1 KB chunk per operand and wave");
    static_assert(NLIVE < 16, "vmcnt(NLIVE) in the low bits of s_waitcnt");

// DMA number Q (0 .. NDMA-1) of a slab, in the order of PS_ISSUE: A_hi / A_lo chunk pairs, then the W chunks
#define PS_DMA_Q(Q, AH, AL, BB, KOFF)                                                                         \
    do {                                                                                                      \
        if ((Q) < 2 * ACH) {                                                                                  \
            if (((Q) & 1) == 0) PS_DMA(rah, &AH[(wave * ACH + (Q) / 2) * 512], va_[(Q) / 2], ka_);             \
            else if (SPLIT) PS_DMA(ral, &AL[(wave * ACH + (Q) / 2) * 512], va_[(Q) / 2], ka_);                 \
        } else {                                                                                              \
            PS_DMA(rw, &BB[(wave * BCH + ((Q) - 2 * ACH)) * 512], b_voff[(Q) - 2 * ACH], (KOFF));              \
        }                                                                                                     \
    } while (0)
#define PS_LDS8(BASE, OFF) (*reinterpret_cast<const half8_t*>(reinterpret_cast<const char*>(BASE) + (OFF)))

// Hi plane only.  Slab S sits in stage (CAH, CB); the DMAs of slab S+1 (if any) are the youngest outstanding ones: wait
// until only those remain, make the landed data visible to every wave, then request every fragment of the slab (both
// 16-wide K chunks) from LDS before the first matrix instruction, so that the LDS latency of the second chunk runs under
// the first chunk's MFMAs, and spread the refill of the stage read at slab S-1 (NAH, NB) over the slab: DMA slot q
// follows the q-th MFMA.
#define PS_STEP(S, CAH, CB, NAH, NB)                                                                                   \
    do {                                                                                                               \
        if ((S) + 1 < nslab) __builtin_amdgcn_s_waitcnt(0x0070 | NLIVE); /* vmcnt(NLIVE) lgkmcnt(0) */                \
        else __builtin_amdgcn_s_waitcnt(0x0070);                         /* vmcnt(0) lgkmcnt(0) */                     \
        __builtin_amdgcn_s_barrier();                                                                                  \
        asm volatile("" ::: "memory");                                                                                 \
        const bool more_ = (S) + 2 < nslab;                                                                            \
        half8_t ah[2][TM], bf[2][TN];                                                                                  \
        _Pragma("unroll") for (int kc = 0; kc < 2; ++kc) {                                                             \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) ah[kc][i] = PS_LDS8(CAH, a_off[i][kc]);                     \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) bf[kc][j] = PS_LDS8(CB, b_off[j][kc]);                      \
        }                                                                                                              \
        if (more_) PS_NEXT_ADDR();                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        int q_ = 0;                                                                                                    \
        _Pragma("unroll") for (int kc = 0; kc < 2; ++kc) {                                                             \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                             \
                _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                       \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[kc][i], bf[kc][j], acc[i][j], 0, 0, 0);       \
                    if (q_ < NDMA) {                                                                                   \
                        __builtin_amdgcn_sched_barrier(0);                                                             \
                        if (more_) PS_DMA_Q(q_, NAH, NAH, NB, ((S) + 2) * (PBK * 2));                                  \
                        __builtin_amdgcn_sched_barrier(0);                                                             \
                    }                                                                                                  \
                    ++q_;                                                                                              \
                }                                                                                                      \
        }                                                                                                              \
        /* tiles with fewer MFMAs than DMA slots (64 x 64: 2 MFMAs, 3 slots): the rest follows the last one */         \
        _Pragma("unroll") for (int q2 = 2 * TM * TN; q2 < NDMA; ++q2)                                                  \
            if (more_) PS_DMA_Q(q2, NAH, NAH, NB, ((S) + 2) * (PBK * 2));                                              \
        asm volatile("" ::: "memory");                                                                                 \
    } while (0)

    const int nslab = p.K / PBK;
    if constexpr (ALTERNATE) {
        static_assert(NDMA == 6, "the alternating schedule is written for the split 8-wave tile");
        constexpr int NH = NDMA / 2;  // DMAs of a slab per 16-wide K chunk and wave, all issued by the chunk's LOAD segment
        const bool grp_b = __builtin_amdgcn_readfirstlane(wave) >= NWAVE / 2;
        half8_t f_ah[TM], f_al[TM], f_bf[TN];  // the fragments of one 16-wide K chunk
// LOAD segment of chunk KC of slab S (stage C*): the chunk's 8 fragment reads, then the wave's NH DMAs of that chunk for
// slab S+2 (stage N*), then every read retired (the stage may be refilled one segment after the barrier that follows)
#define PP_LOADSEG(S, KC, CAH, CAL, CB, NAH, NAL, NB)                                           \
    do {                                                                                        \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) f_bf[j] = PS_LDS8(CB, b_off[j][KC]);     \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                        \
            f_ah[i] = PS_LDS8(CAH, a_off[i][KC]);                                               \
            f_al[i] = PS_LDS8(CAL, a_off[i][KC]);                                               \
        }                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        if ((S) + 2 < nslab) {                                                                  \
            if ((KC) == 0) PS_NEXT_ADDR();                                                      \
            _Pragma("unroll") for (int q = (KC) * NH; q < (KC) * NH + NH; ++q) PS_DMA_Q(q, NAH, NAL, NB, ((S) + 2) * (PBK * 2)); \
        }                                                                                       \
        __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0), vmcnt untouched */                   \
        __builtin_amdgcn_sched_barrier(0);                                                      \
    } while (0)
// COMPUTE segment: the chunk's hi products of all eight accumulators, then the lo products (an accumulator's two instructions
// are eight issues apart; its order hi, lo is the one of every other schedule)
#define PP_COMPUTE()                                                                                               \
    do {                                                                                                           \
        __builtin_amdgcn_s_setprio(1);                                                                             \
        _Pragma("unroll") for (int h_ = 0; h_ < 2; ++h_)                                                           \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                         \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h_ == 0 ? f_ah[i] : f_al[i], f_bf[j], acc[i][j], 0, 0, 0); \
        __builtin_amdgcn_s_setprio(0);                                                                             \
    } while (0)
#define PP_BARRIER()                            \
    do {                                        \
        __builtin_amdgcn_sched_barrier(0);      \
        __builtin_amdgcn_s_barrier();           \
        asm volatile("" ::: "memory");          \
        __builtin_amdgcn_sched_barrier(0);      \
    } while (0)
// slab S (stage C*; N* = stage of slab S+2, the one slab S-1 sat in): four segments.  ROLE_B = false (waves 0-3): load /
// compute / load / compute; true (waves 4-7): compute (the previous chunk) / load / compute / load.  The two roles are two
// separate loops (no control flow joins inside the K loop: the 128 accumulator registers stay where they are); both execute
// the same number of barriers.  At the end of the step both roles have issued all 6 DMAs of slab S+2, and slab S+1 must
// have landed.
#define PP_STEP(ROLE_B, S, CAH, CAL, CB, NAH, NAL, NB)                                          \
    do {                                                                                        \
        if (!(ROLE_B)) PP_LOADSEG(S, 0, CAH, CAL, CB, NAH, NAL, NB);                            \
        else if ((S) > 0) PP_COMPUTE();                                                         \
        PP_BARRIER();                                                                           \
        if (!(ROLE_B)) PP_COMPUTE();                                                            \
        else PP_LOADSEG(S, 0, CAH, CAL, CB, NAH, NAL, NB);                                      \
        PP_BARRIER();                                                                           \
        if (!(ROLE_B)) PP_LOADSEG(S, 1, CAH, CAL, CB, NAH, NAL, NB);                            \
        else PP_COMPUTE();                                                                      \
        PP_BARRIER();                                                                           \
        if (!(ROLE_B)) PP_COMPUTE();                                                            \
        else PP_LOADSEG(S, 1, CAH, CAL, CB, NAH, NAL, NB);                                      \
        if ((S) + 2 < nslab) __builtin_amdgcn_s_waitcnt(0x0076); /* vmcnt(6) lgkmcnt(0) */      \
        else __builtin_amdgcn_s_waitcnt(0x0070);                                                \
        PP_BARRIER();                                                                           \
    } while (0)
#define PP_LOOP(ROLE_B)                                                                         \
    do {                                                                                        \
        for (int s = 0; s < nslab; s += 3) {                                                    \
            PP_STEP(ROLE_B, s, sAh0, sAl0, sB0, sAh2, sAl2, sB2);                               \
            if (s + 1 < nslab) PP_STEP(ROLE_B, s + 1, sAh1, sAl1, sB1, sAh0, sAl0, sB0);        \
            if (s + 2 < nslab) PP_STEP(ROLE_B, s + 2, sAh2, sAl2, sB2, sAh1, sAl1, sB1);        \
        }                                                                                       \
        if (ROLE_B) PP_COMPUTE(); /* the last chunk of waves 4-7 */                             \
    } while (0)
        PS_ISSUE(sAh0, sAl0, sB0, 0);
        if (nslab > 1) PS_ISSUE(sAh1, sAl1, sB1, PBK * 2);
        if (nslab > 1) __builtin_amdgcn_s_waitcnt(0x0076);
        else __builtin_amdgcn_s_waitcnt(0x0070);
        PP_BARRIER();
        if (grp_b) PP_LOOP(true);
        else PP_LOOP(false);
#undef PP_LOOP
#undef PP_STEP
#undef PP_BARRIER
#undef PP_LOADSEG
#undef PP_COMPUTE
    } else if constexpr (MID_BARRIER) {
        constexpr int NH = NDMA / 2;  // DMAs of a slab issued in the second half of step s-3; the rest in the first half of step s-2
        half8_t c_ah[TM], c_al[TM], c_bf[TN];  // chunk-0 fragments of the current slab, carried from the previous step
#define PS_READ_C0(AH, AL, BB)                                                                  \
    do {                                                                                        \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                        \
            c_ah[i] = PS_LDS8(AH, a_off[i][0]);                                                 \
            c_al[i] = PS_LDS8(AL, a_off[i][0]);                                                 \
        }                                                                                       \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) c_bf[j] = PS_LDS8(BB, b_off[j][0]);      \
    } while (0)
// C* = stage of slab S (and of S+3), N* = stage of S+1, O* = stage of S+2
#define PS_HSTEP(S, CAH, CAL, CB, NAH, NAL, NB, OAH, OAL, OB)                                                          \
    do {                                                                                                               \
        half8_t ah1[TM], al1[TM], bf1[TN];                                                                             \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                               \
            ah1[i] = PS_LDS8(CAH, a_off[i][1]);                                                                        \
            al1[i] = PS_LDS8(CAL, a_off[i][1]);                                                                        \
        }                                                                                                              \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) bf1[j] = PS_LDS8(CB, b_off[j][1]);                              \
        const bool iss2_ = (S) + 2 < nslab;                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        int q_ = NH;                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                 \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                           \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(c_ah[i], c_bf[j], acc[i][j], 0, 0, 0);               \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(c_al[i], c_bf[j], acc[i][j], 0, 0, 0);               \
                if (q_ < NDMA) {                                                                                       \
                    __builtin_amdgcn_sched_barrier(0);                                                                 \
                    if (iss2_) PS_DMA_Q(q_, OAH, OAL, OB, ((S) + 2) * (PBK * 2));                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                 \
                }                                                                                                      \
                ++q_;                                                                                                  \
            }                                                                                                          \
        _Pragma("unroll") for (int q2 = NH + TM * TN; q2 < NDMA; ++q2)                                                 \
            if (iss2_) PS_DMA_Q(q2, OAH, OAL, OB, ((S) + 2) * (PBK * 2));                                              \
        if ((S) + 1 < nslab) {                                                                                         \
            if (iss2_) __builtin_amdgcn_s_waitcnt(NDMA == 6 ? 0x0076 : 0x0073); /* vmcnt(6 | 3) lgkmcnt(0) */          \
            else __builtin_amdgcn_s_waitcnt(0x0070);                            /* vmcnt(0) lgkmcnt(0) */              \
            __builtin_amdgcn_s_barrier();                                                                              \
            asm volatile("" ::: "memory");                                                                             \
            PS_READ_C0(NAH, NAL, NB);                                                                                  \
        }                                                                                                              \
        const bool iss3_ = (S) + 3 < nslab;                                                                            \
        if (iss3_) PS_NEXT_ADDR();                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        q_ = 0;                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                 \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                           \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1[i], bf1[j], acc[i][j], 0, 0, 0);                 \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al1[i], bf1[j], acc[i][j], 0, 0, 0);                 \
                if (q_ < NH) {                                                                                         \
                    __builtin_amdgcn_sched_barrier(0);                                                                 \
                    if (iss3_) PS_DMA_Q(q_, CAH, CAL, CB, ((S) + 3) * (PBK * 2));                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                 \
                }                                                                                                      \
                ++q_;                                                                                                  \
            }                                                                                                          \
        asm volatile("" ::: "memory");                                                                                 \
    } while (0)

        // prologue: slabs 0 and 1 whole, the first NH DMAs of slab 2; slab 0 must have landed before its fragments are read
        PS_ISSUE(sAh0, sAl0, sB0, 0);
        if (nslab > 1) PS_ISSUE(sAh1, sAl1, sB1, PBK * 2);
        if (nslab > 2) {
            PS_NEXT_ADDR();
#pragma unroll
            for (int q = 0; q < NH; ++q) PS_DMA_Q(q, sAh2, sAl2, sB2, 2 * (PBK * 2));
        }
        if (nslab > 2) __builtin_amdgcn_s_waitcnt(NDMA == 6 ? 0x0079 : 0x0074);       // vmcnt(NDMA + NH)
        else if (nslab > 1) __builtin_amdgcn_s_waitcnt(NDMA == 6 ? 0x0076 : 0x0073);  // vmcnt(NDMA)
        else __builtin_amdgcn_s_waitcnt(0x0070);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        PS_READ_C0(sAh0, sAl0, sB0);
        for (int s = 0; s < nslab; s += 3) {
            PS_HSTEP(s, sAh0, sAl0, sB0, sAh1, sAl1, sB1, sAh2, sAl2, sB2);
            if (s + 1 < nslab) PS_HSTEP(s + 1, sAh1, sAl1, sB1, sAh2, sAl2, sB2, sAh0, sAl0, sB0);
            if (s + 2 < nslab) PS_HSTEP(s + 2, sAh2, sAl2, sB2, sAh0, sAl0, sB0, sAh1, sAl1, sB1);
        }
#undef PS_HSTEP
#undef PS_READ_C0
    } else {
        PS_ISSUE(sAh0, sAl0, sB0, 0);
        if (nslab > 1) PS_ISSUE(sAh1, sAl1, sB1, PBK * 2);
        for (int s = 0; s < nslab; s += 3) {
            PS_STEP(s, sAh0, sB0, sAh2, sB2);
            if (s + 1 < nslab) PS_STEP(s + 1, sAh1, sB1, sAh0, sB0);
            if (s + 2 < nslab) PS_STEP(s + 2, sAh2, sB2, sAh1, sB1);
        }
    }
#undef PS_STEP
#undef PS_LDS8
#undef PS_DMA_Q
#undef PS_NEXT_ADDR
#undef PS_ISSUE
#undef PS_DMA

    // ---- epilogue through LDS: accumulators (column per lane) -> row-major tile of this wave -> 16-byte rows ----
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();  // every wave is done reading the last stage
    asm volatile("" ::: "memory");
    float* ep = reinterpret_cast<float*>(smem) + wave * (WM * EP_LD);
    const int m0w = m0 + wm * WM;
    // the wave's tile leaves in passes of EPN columns through its private LDS region (the LDS queue of a wave is in
    // order: a pass's writes follow the previous pass's reads)
    float am_best = -INFINITY;  // AMAX: lane r < WM scans row r of the wave's tile, columns ascending over the passes
    int am_idx = 0x7fffffff;
    // SCORE: lane r < WM keeps the record of row r over the wave's WN columns, columns ascending over the passes: running
    // maximum (am_best, its lowest column am_idx), sum of exp(v - maximum), sum of v, v at the row's target column
    float sc_sum = 0.f, sc_sumv = 0.f, sc_vt = 0.f;
    int sc_tgt = -1;
    if constexpr (SCORE && !CAND) {
        if (lane < WM && m0w + lane < p.M) sc_tgt = sc.target[m0w + lane];
    }
    // CAND: the candidates [cd_j, cd_j1) of the sorted list lie in the wave's columns [n0 + wn * WN, + WN): two binary searches
    // per wave, wave-uniform (scalar loads); the passes then consume them in ascending order
    int cd_j = 0, cd_j1 = 0;
    if constexpr (CAND) {
        const int c_lo = __builtin_amdgcn_readfirstlane(n0 + wn * WN);
        int lo = 0, hi = cd.n_cand;  // first candidate >= c_lo
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cd.cand[mid] < c_lo) lo = mid + 1;
            else hi = mid;
        }
        cd_j = lo;
        hi = cd.n_cand;  // first candidate >= c_lo + WN
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cd.cand[mid] < c_lo + WN) lo = mid + 1;
            else hi = mid;
        }
        cd_j1 = lo;
    }
    auto pass = [&](auto hc) {  // compile-time pass number: the accumulator registers are indexed by constants
        constexpr int h = decltype(hc)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < EPN / 32; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ep[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * EP_LD + j * 32 + (lane & 31)] = acc[i][h * (EPN / 32) + j][r];
        const int n0w = n0 + wn * WN + h * EPN;
        if constexpr (AMAX) {
            if (lane < WM) {
                const float* row = ep + lane * EP_LD;
#pragma unroll
                for (int c4 = 0; c4 < EPN / 4; ++c4) {
                    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(row + 4 * c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = n0w + 4 * c4 + e;
                        if (col < p.N) {
                            const float v = (a[e] + (p.bias ? p.bias[col] : 0.f)) * p.alpha;  // = ps_epilogue's value with ACT_NONE
                            if (v > am_best) {  // strictly: the lowest column among equal values stays
                                am_best = v;
                                am_idx = col;
                            }
                        }
                    }
                }
            }
            return;
        }
        if constexpr (SCORE) {
            if (lane < WM && n0w < p.N) {  // (a pass without a column below N leaves the record as it is)
                const float* row = ep + lane * EP_LD;
                const float mx_old = am_best;
                // first the pass's maximum (and everything that needs no maximum), then the exponentials against it: the value
                // is formed twice by the same instructions, the tile is read from LDS twice
#pragma unroll
                for (int c4 = 0; c4 < EPN / 4; ++c4) {
                    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(row + 4 * c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = n0w + 4 * c4 + e;
                        if (col < p.N) {
                            const float v = (a[e] + (p.bias ? p.bias[col] : 0.f)) * p.alpha;  // = ps_epilogue's value with ACT_NONE
                            sc_sumv += v;
                            if (col == sc_tgt) sc_vt = v;
                            if (v > am_best) {  // strictly: the lowest column among equal values stays
                                am_best = v;
                                am_idx = col;
                            }
                        }
                    }
                }
                // what the earlier passes summed was relative to their maximum (pass 0 has nothing to rescale)
                if (h > 0) sc_sum *= expf(mx_old - am_best);
#pragma unroll
                for (int c4 = 0; c4 < EPN / 4; ++c4) {
                    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(row + 4 * c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = n0w + 4 * c4 + e;
                        if (col < p.N) {
                            const float v = (a[e] + (p.bias ? p.bias[col] : 0.f)) * p.alpha;
                            sc_sum += expf(v - am_best);
                        }
                    }
                }
            }
            if constexpr (CAND) {
                // the candidates inside this pass's columns (all below N: the list is checked on the host), out of the tile
                // that still sits in LDS: lane r reads row r at the candidate's column and forms v as above
                while (cd_j < cd_j1) {
                    const int col = cd.cand[cd_j];
                    if (col >= n0w + EPN) break;
                    if (lane < WM && m0w + lane < p.M) {
                        const float a = ep[lane * EP_LD + (col - n0w)];
                        const float v = (a + (p.bias ? p.bias[col] : 0.f)) * p.alpha;
                        cd.v[(int64_t)(m0w + lane) * cd.n_cand + cd_j] = v;
                    }
                    ++cd_j;
                }
            }
            return;
        }
        if constexpr (GLU) {
            ps_epilogue_glu<WM, EPN, EP_LD>(p, ep, m0w, n0w, lane);
            return;
        }
        if (p.act == ACT_NONE) ps_epilogue<WM, EPN, EP_LD, ACT_NONE>(p, ep, m0w, n0w, lane);
        else if (p.act == ACT_RELU) ps_epilogue<WM, EPN, EP_LD, ACT_RELU>(p, ep, m0w, n0w, lane);
        else if (p.act == ACT_SILU) ps_epilogue<WM, EPN, EP_LD, ACT_SILU>(p, ep, m0w, n0w, lane);
        else ps_epilogue<WM, EPN, EP_LD, ACT_TANH>(p, ep, m0w, n0w, lane);
    };
    static_assert(WN % EPN == 0 && WN / EPN >= 1 && WN / EPN <= 4, "one to four epilogue passes");
    pass(std::integral_constant<int, 0>{});
    if constexpr (WN / EPN > 1) pass(std::integral_constant<int, 1>{});
    if constexpr (WN / EPN > 2) pass(std::integral_constant<int, 2>{});
    if constexpr (WN / EPN > 3) pass(std::integral_constant<int, 3>{});
    if constexpr (AMAX) {
        const int64_t m = m0w + lane;
        if (lane < WM && m < p.M) p.amax[m * p.amax_ld + tn * WGN + wn] = make_float2(am_best, __int_as_float(am_idx));
    }
    if constexpr (SCORE) {
        const int64_t m = m0w + lane;
        const int r = tn * WGN + wn;  // record number = (first column of the wave) / WN; records without a column below N do not exist
        if (lane < WM && m < p.M && r < sc.ld) {
            float2* out = reinterpret_cast<float2*>(sc.rec + (m * sc.ld + r) * SCORE_REC_FLOATS);
            out[0] = make_float2(am_best, sc_sum);
            out[1] = make_float2(sc_sumv, sc_vt);
            out[2] = make_float2(__int_as_float(am_idx), 0.f);
        }
    }
