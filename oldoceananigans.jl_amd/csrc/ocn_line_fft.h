// ocn_line_fft.h -- the power-of-two line FFTs in LDS and the kernels built on nothing else: zline_solve_kernel, strided_line_fft_kernel,
// xline_solve_kernel, paired_zline_r2c_kernel / paired_zline_c2r_kernel. gfx950 / wave64. Needs double2 and nothing else of the project.
//
// ONE implementation of the arithmetic, in three layers:
//   * the register butterflies dif_butterfly2 / dit_butterfly2 / dif_butterfly4 / dit_butterfly4 -- the place to change a butterfly;
//   * the index formulas line_idx2 / line_dif_idx4 / line_dit_idx4 (which points, which twiddles butterfly q of a stage takes) and the
//     stage bodies line_*_apply* (load through an accessor n -> double2&, butterfly, store) -- the place to change a stage;
//   * two drivers of the stages: LineFFT<ZL, NC> (line length at compile time, twiddles preloaded a stage ahead) and
//     lds_fft_forward / lds_fft_inverse (any length 2^logn, twiddles loaded per butterfly) on either LDS layout.
// Every path runs the same operations on the same operands in the same order (the build has -ffp-contract=off): bit-identical results.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double2 line_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 line_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 line_cmul(double2 v, double2 w) { return make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x); }     // v * w
__device__ __forceinline__ double2 line_cmulc(double2 v, double2 w) { return make_double2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y); }    // v * conj(w)

// ---------------------------------------------------------------------------------------------------------------------
// The butterflies, in registers and in place. Decimation in frequency (forward, twiddle w = exp(-2πi m / N) behind the difference) and
// decimation in time (inverse, conjugate twiddle in front of the sum); a radix-4 butterfly is two radix-2 stages fused.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dif_butterfly2(double2 &xa, double2 &xb, double2 w) {
    const double2 s = line_add(xa, xb);
    xb = line_cmul(line_sub(xa, xb), w);
    xa = s;
}
__device__ __forceinline__ void dit_butterfly2(double2 &xa, double2 &xb, double2 w) {
    const double2 u = line_cmulc(xb, w);
    xb = line_sub(xa, u);
    xa = line_add(xa, u);
}
// x = the points a, a + h/2, a + h, a + 3h/2 (in this order)
__device__ __forceinline__ void dif_butterfly4(double2 (&x)[4], double2 wa, double2 wb, double2 wc) {
    const double2 y0 = line_add(x[0], x[2]), y2 = line_cmul(line_sub(x[0], x[2]), wa);
    const double2 y1 = line_add(x[1], x[3]), y3 = line_cmul(line_sub(x[1], x[3]), wb);
    x[0] = line_add(y0, y1);
    x[1] = line_cmul(line_sub(y0, y1), wc);
    x[2] = line_add(y2, y3);
    x[3] = line_cmul(line_sub(y2, y3), wc);
}
// x = the points a, a + h, a + 2h, a + 3h (in this order)
__device__ __forceinline__ void dit_butterfly4(double2 (&x)[4], double2 wa, double2 wb, double2 wc) {
    const double2 t1 = line_cmulc(x[1], wa), t3 = line_cmulc(x[3], wa);
    const double2 y0 = line_add(x[0], t1), y1 = line_sub(x[0], t1);
    const double2 y2 = line_add(x[2], t3), y3 = line_sub(x[2], t3);
    const double2 u2 = line_cmulc(y2, wb), u3 = line_cmulc(y3, wc);
    x[0] = line_add(y0, u2);
    x[2] = line_sub(y0, u2);
    x[1] = line_add(y1, u3);
    x[3] = line_sub(y1, u3);
}

// ---------------------------------------------------------------------------------------------------------------------
// Butterfly q of a stage at span h with twiddle stride st: the points it works on (p) and its twiddles (indices into tw[m] =
// exp(-2πi m / N), m < N/2). jj is masked, so every twiddle index stays under N/2 for ANY q: a thread without a butterfly (q past the
// end of the stage) may still load its twiddles.
// ---------------------------------------------------------------------------------------------------------------------
struct LineIdx2 { int p[2], w; };
struct LineIdx4 { int p[4], wa, wb, wc; };
// radix-2, DIF and DIT alike: blocks of 2h points, jj < h
__device__ __forceinline__ LineIdx2 line_idx2(int q, int h, int st) {
    const int jj = q & (h - 1), a = ((q - jj) << 1) + jj;
    return {{a, a + h}, jj * st};
}
// radix-4 DIF (the radix-2 stages at spans h and h/2): blocks of 2h points, jj < h/2
__device__ __forceinline__ LineIdx4 line_dif_idx4(int q, int h, int st) {
    const int h2 = h >> 1, jj = q & (h2 - 1), a = ((q - jj) << 2) + jj;
    return {{a, a + h2, a + h, a + h + h2}, jj * st, (jj + h2) * st, jj * 2 * st};
}
// radix-4 DIT (the radix-2 stages at spans h and 2h): blocks of 4h points, jj < h
__device__ __forceinline__ LineIdx4 line_dit_idx4(int q, int h, int st) {
    const int jj = q & (h - 1), a = ((q - jj) << 2) + jj;
    return {{a, a + h, a + 2 * h, a + 3 * h}, jj * st, jj * (st >> 1), (jj + h) * (st >> 1)};
}

// The two LDS layouts, as accessors point n of a line -> double2&:
// interleaved, ZL lines side by side: zbuf[n * ZL + il]
template <int ZL> struct InterleavedLine {
    double2 *zbuf;
    int il;
    __device__ __forceinline__ double2 &operator()(int n) const { return zbuf[n * ZL + il]; }
};
// whole lines one after the other: line[n], line = zbuf + (ln << logn)
struct ContiguousLine {
    double2 *line;
    __device__ __forceinline__ double2 &operator()(int n) const { return line[n]; }
};

// one butterfly of a stage: load, butterfly, store
template <class Z> __device__ __forceinline__ void line_dif_apply2(Z z, const LineIdx2 &i, double2 w) {
    double2 xa = z(i.p[0]), xb = z(i.p[1]);
    dif_butterfly2(xa, xb, w);
    z(i.p[0]) = xa;
    z(i.p[1]) = xb;
}
template <class Z> __device__ __forceinline__ void line_dit_apply2(Z z, const LineIdx2 &i, double2 w) {
    double2 xa = z(i.p[0]), xb = z(i.p[1]);
    dit_butterfly2(xa, xb, w);
    z(i.p[0]) = xa;
    z(i.p[1]) = xb;
}
template <class Z> __device__ __forceinline__ void line_dif_apply4(Z z, const LineIdx4 &i, double2 wa, double2 wb, double2 wc) {
    double2 x[4] = {z(i.p[0]), z(i.p[1]), z(i.p[2]), z(i.p[3])};
    dif_butterfly4(x, wa, wb, wc);
#pragma unroll
    for (int m = 0; m < 4; ++m) z(i.p[m]) = x[m];
}
template <class Z> __device__ __forceinline__ void line_dit_apply4(Z z, const LineIdx4 &i, double2 wa, double2 wb, double2 wc) {
    double2 x[4] = {z(i.p[0]), z(i.p[1]), z(i.p[2]), z(i.p[3])};
    dit_butterfly4(x, wa, wb, wc);
#pragma unroll
    for (int m = 0; m < 4; ++m) z(i.p[m]) = x[m];
}

// ---------------------------------------------------------------------------------------------------------------------
// The LDS line kernels below (zline_solve_kernel, strided_line_fft_kernel) at a line length known when they are compiled: NC points,
// E = NC / KQ = 1, 2, 4, 8 or 16 of them per thread (KQ = 256 / ZL k-rows per pass). The generic loops have run-time trip counts, and the
// compiler serialises them: one global_load_dwordx4, s_waitcnt vmcnt(0), one ds_write_b128 per iteration -- E HBM round trips one after
// the other with 16 B per lane in flight --, and every butterfly waits for its own twiddle loads. Here
//  * a thread issues ALL E loads of its part of the line back to back, and only then writes them to LDS; a lane past the last column
//    loads its workgroup's first column instead (a clamped address, no branch between the loads) and stores zeros;
//  * the twiddles of a butterfly stage are in registers before the stage starts: those of the first stage are loaded behind the data
//    loads, those of every later stage in front of the LDS reads of the stage before it (LDS stays at NC x ZL x 16 B: the same
//    workgroups per CU, and 1024 x 4 lines already take the 64 KB a workgroup may ask for).
// Same values, same operations in the same order as the generic loops (the build has -ffp-contract=off): bit-identical results.
// OCN_LINE_IN_FLIGHT=0 sends every line length back to the generic loops -- for A/B timing only (tools/ab_build.sh).
// ---------------------------------------------------------------------------------------------------------------------
#ifndef OCN_LINE_IN_FLIGHT
#define OCN_LINE_IN_FLIGHT 1
#endif
constexpr int line_ilog2(int n) { return n <= 1 ? 0 : 1 + line_ilog2(n >> 1); }
// waves per SIMD the fixed-length kernels must leave room for: a 32 KB line buffer fits five times into a CU's 160 KB of LDS, and five
// workgroups of four waves are five waves per SIMD (<= 96 VGPRs); every other shape is left to the compiler
constexpr int line_min_waves(int zl, int nc) { return nc * zl * (int)sizeof(double2) == 32768 ? 5 : 1; }

template <int ZL, int NC>
struct LineFFT {
    static constexpr int KQ = 256 / ZL, E = NC / KQ, HALF = NC >> 1, QUARTER = NC >> 2, LOGN = line_ilog2(NC);
    static constexpr int ODD = LOGN & 1, NS4 = LOGN >> 1;                         // one radix-2 stage when log2 NC is odd, NS4 radix-4 stages
    static constexpr int I2 = (HALF + KQ - 1) / KQ, I4 = (QUARTER + KQ - 1) / KQ; // butterflies per thread and stage
    static_assert(NC == E * KQ && (NC & (NC - 1)) == 0 && E >= 1 && E <= 16, "line length: 1, 2, 4, 8 or 16 points per thread");
    struct Tw2 { double2 w[I2]; };
    struct Tw4 { double2 a[I4], b[I4], c[I4]; };

    // thread (il, kq) holds points kq, kq + KQ, ...: E loads back to back from p (point kq of its column), `stride` elements apart
    static __device__ __forceinline__ void load(const double2 *p, long stride, double2 (&r)[E]) {
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] = p[stride * (e * KQ)];
    }
    // the twiddle loads of a thread without a butterfly (q past the loop's end) are in bounds: see the index formulas
    // forward = decimation in frequency: [radix-2 at span NC/2,] radix-4 stage s at h = (NC/2 >> ODD) >> 2s, twiddle stride st = (1 << ODD) << 2s
    static __device__ __forceinline__ void dif_tw2(const double2 *tw, int kq, Tw2 &t) {
#pragma unroll
        for (int it = 0; it < I2; ++it) t.w[it] = tw[line_idx2(kq + it * KQ, HALF, 1).w];
    }
    static __device__ __forceinline__ void dif_stage2(double2 *zbuf, int il, int kq, const Tw2 &t) {
#pragma unroll
        for (int it = 0; it < I2; ++it) {
            const int q = kq + it * KQ;
            if (HALF % KQ == 0 || q < HALF) line_dif_apply2(InterleavedLine<ZL>{zbuf, il}, line_idx2(q, HALF, 1), t.w[it]);
        }
    }
    static __device__ __forceinline__ void dif_tw4(const double2 *tw, int kq, int s, Tw4 &t) {
        const int h = (HALF >> ODD) >> (2 * s), st = (1 << ODD) << (2 * s);
#pragma unroll
        for (int it = 0; it < I4; ++it) {
            const LineIdx4 i = line_dif_idx4(kq + it * KQ, h, st);
            t.a[it] = tw[i.wa];
            t.b[it] = tw[i.wb];
            t.c[it] = tw[i.wc];
        }
    }
    static __device__ __forceinline__ void dif_stage4(double2 *zbuf, int il, int kq, int s, const Tw4 &t) {
        const int h = (HALF >> ODD) >> (2 * s), st = (1 << ODD) << (2 * s);
#pragma unroll
        for (int it = 0; it < I4; ++it) {
            const int q = kq + it * KQ;
            if (QUARTER % KQ == 0 || q < QUARTER) line_dif_apply4(InterleavedLine<ZL>{zbuf, il}, line_dif_idx4(q, h, st), t.a[it], t.b[it], t.c[it]);
        }
    }
    // twiddles of the first forward stage(s): call behind the data loads
    static __device__ __forceinline__ void dif_first_tw(const double2 *tw, int kq, Tw2 &t2, Tw4 &t4) {
        if (ODD) dif_tw2(tw, kq, t2);
        dif_tw4(tw, kq, 0, t4);
    }
    // the line is in LDS (barrier passed) -> the line after the radix-4 stages [0, S_END) (barrier passed); S_END = NS4: the whole transform,
    // the line in bit-reversed order. t: the twiddles of stage 0 on entry, those of stage S_END on return (if there is one). `before_last`
    // runs in front of the LDS reads of the last stage done here: the place for loads the caller needs right after it
    template <int S_END, class F>
    static __device__ __forceinline__ void forward_to(double2 *zbuf, const double2 *tw, int il, int kq, const Tw2 &t2, Tw4 &t, F &&before_last) {
        if (ODD) {
            dif_stage2(zbuf, il, kq, t2);
            __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < S_END; ++s) {
            Tw4 next;
            if (s + 1 < NS4) dif_tw4(tw, kq, s + 1, next);
            if (s + 1 == S_END) before_last();
            dif_stage4(zbuf, il, kq, s, t);
            __syncthreads();
            if (s + 1 < NS4) t = next;
        }
    }
    static __device__ __forceinline__ void forward(double2 *zbuf, const double2 *tw, int il, int kq, const Tw2 &t2, Tw4 t) {
        forward_to<NS4>(zbuf, tw, il, kq, t2, t, [] {});
    }
    // inverse = decimation in time, conjugate twiddles: radix-4 stage s at h = 1 << 2s, st = NC/2 >> 2s [, radix-2 at span NC/2, st = 1]
    static __device__ __forceinline__ void dit_tw4(const double2 *tw, int kq, int s, Tw4 &t) {
        const int h = 1 << (2 * s), st = HALF >> (2 * s);
#pragma unroll
        for (int it = 0; it < I4; ++it) {
            const LineIdx4 i = line_dit_idx4(kq + it * KQ, h, st);
            t.a[it] = tw[i.wa];
            t.b[it] = tw[i.wb];
            t.c[it] = tw[i.wc];
        }
    }
    static __device__ __forceinline__ void dit_stage4(double2 *zbuf, int il, int kq, int s, const Tw4 &t) {
        const int h = 1 << (2 * s), st = HALF >> (2 * s);
#pragma unroll
        for (int it = 0; it < I4; ++it) {
            const int q = kq + it * KQ;
            if (QUARTER % KQ == 0 || q < QUARTER) line_dit_apply4(InterleavedLine<ZL>{zbuf, il}, line_dit_idx4(q, h, st), t.a[it], t.b[it], t.c[it]);
        }
    }
    static __device__ __forceinline__ void dit_tw2(const double2 *tw, int kq, Tw2 &t) { dif_tw2(tw, kq, t); }      // h = NC/2, st = 1 again
    static __device__ __forceinline__ void dit_stage2(double2 *zbuf, int il, int kq, const Tw2 &t) {
#pragma unroll
        for (int it = 0; it < I2; ++it) {
            const int q = kq + it * KQ;
            if (HALF % KQ == 0 || q < HALF) line_dit_apply2(InterleavedLine<ZL>{zbuf, il}, line_idx2(q, HALF, 1), t.w[it]);
        }
    }
    // the line after the radix-4 stages [0, S_BEGIN) is in LDS (barrier passed; S_BEGIN = 0: the bit-reversed line), t = dit_tw4 of stage
    // S_BEGIN -> the line in natural order (barrier passed)
    template <int S_BEGIN = 0>
    static __device__ __forceinline__ void inverse(double2 *zbuf, const double2 *tw, int il, int kq, Tw4 t) {
        Tw2 t2;
        if (ODD && S_BEGIN == NS4) dit_tw2(tw, kq, t2);
#pragma unroll
        for (int s = S_BEGIN; s < NS4; ++s) {
            Tw4 next;
            if (s + 1 < NS4) dit_tw4(tw, kq, s + 1, next);
            else if (ODD) dit_tw2(tw, kq, t2);
            dit_stage4(zbuf, il, kq, s, t);
            __syncthreads();
            if (s + 1 < NS4) t = next;
        }
        if (ODD) {
            dit_stage2(zbuf, il, kq, t2);
            __syncthreads();
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The same transforms at any line length N = 2^logn: run-time trip counts, twiddles loaded per butterfly. The lines of a workgroup of 256
// threads, in either layout, hand out the butterflies of a stage: each(per_line, r, f) calls f(accessor of a line, q) for the thread's share
// of the per_line = N >> r butterflies of every line (r = 1: radix-2, r = 2: radix-4).
// ---------------------------------------------------------------------------------------------------------------------
// zbuf[N][ZL]: thread (il, kq) takes q = kq, kq + KQ, ... of line il
template <int ZL> struct InterleavedLines {
    double2 *zbuf;
    int il, kq;
    template <class F> __device__ __forceinline__ void each(int per_line, int r, F &&f) const {
        for (int q = kq; q < per_line; q += 256 / ZL) f(InterleavedLine<ZL>{zbuf, il}, q);
    }
};
// zbuf[L][N]: thread tid takes e = tid, tid + 256, ... of the L * per_line butterflies, line e / per_line
struct ContiguousLines {
    double2 *zbuf;
    int L, logn;
    template <class F> __device__ __forceinline__ void each(int per_line, int r, F &&f) const {
        for (int e = threadIdx.x; e < L * per_line; e += 256) {
            const int ln = e >> (logn - r), q = e & (per_line - 1);
            f(ContiguousLine{zbuf + (ln << logn)}, q);
        }
    }
};
// forward radix-4 DIF (natural order in, frequency f at position bitreverse(f) out): spans N/2, N/4, ..., 1; two radix-2 stages are fused
// in registers (radix-4 butterflies: half the LDS traffic and barriers), preceded by one radix-2 stage when log2 N is odd.
// The line is in LDS (barrier passed) on entry and on return.
template <class Lines> __device__ __forceinline__ void lds_fft_forward(const Lines &lines, const double2 *tw, int N, int logn) {
    const int half = N >> 1, quarter = N >> 2;
    int h = half, st = 1;
    if (logn & 1) {
        lines.each(half, 1, [=](auto z, int q) {
            const LineIdx2 i = line_idx2(q, h, st);
            line_dif_apply2(z, i, tw[i.w]);
        });
        __syncthreads();
        h >>= 1; st <<= 1;
    }
    for (; h >= 2; h >>= 2, st <<= 2) {
        lines.each(quarter, 2, [=](auto z, int q) {
            const LineIdx4 i = line_dif_idx4(q, h, st);
            line_dif_apply4(z, i, tw[i.wa], tw[i.wb], tw[i.wc]);
        });
        __syncthreads();
    }
}
// inverse radix-4 DIT (frequency f at position bitreverse(f) in, natural order out, unnormalised): spans 1, 2, ..., N/2, conjugate
// twiddles, fused in pairs; one radix-2 stage is left when log2 N is odd. The radix-4 stages are counted: an exit test on h itself
// ((h << 1) <= N/2) is 8h after the increment, the same value as the offset of point a + 2h at ZL = 4, and the compiler, merging the
// two, kept h and st of that instantiation in vector registers.
template <class Lines> __device__ __forceinline__ void lds_fft_inverse(const Lines &lines, const double2 *tw, int N, int logn) {
    const int half = N >> 1, quarter = N >> 2;
    int h = 1, st = half;
    for (int s = logn >> 1; s > 0; --s, h <<= 2, st >>= 2) {
        lines.each(quarter, 2, [=](auto z, int q) {
            const LineIdx4 i = line_dit_idx4(q, h, st);
            line_dit_apply4(z, i, tw[i.wa], tw[i.wb], tw[i.wc]);
        });
        __syncthreads();
    }
    if (logn & 1) {                           // h == half here
        lines.each(half, 1, [=](auto z, int q) {
            const LineIdx2 i = line_idx2(q, h, st);
            line_dit_apply2(z, i, tw[i.w]);
        });
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused z pass of the FFT-based Poisson solve on the Hermitian half spectrum (Nxs, Ny, Nz), z Periodic, Nz a power of two:
// forward FFT along z, ϕ̂ = -b̂ / (λx + λy + λz) (fft_based_poisson_solver.jl:108-118), inverse FFT along z -- ONE pass over the
// array instead of three (rocFFT column transform, divide kernel, rocFFT column transform). A workgroup holds ZL z-lines
// (consecutive in x: 128-B rows) in LDS. Forward = radix-2 decimation in frequency (natural -> bit-reversed order), the divide
// runs in bit-reversed order, inverse = radix-2 decimation in time (bit-reversed -> natural): in place, no reordering pass.
// tw[m] = exp(-2πi m / Nz), m < Nz/2 (host-computed). `scale` folds the normalisation of the whole 3-D inverse transform.
// ---------------------------------------------------------------------------------------------------------------------
// NC > 0: Nz = NC at compile time (LineFFT above); NC = 0: any Nz = 2^logn, the generic loops.
template <int ZL, int NC = 0>
__global__ void __launch_bounds__(256, line_min_waves(ZL, NC)) zline_solve_kernel(double2 *hc, const double2 *tw, const double *lx, const double *ly,
                                                          const double *lz, int Nxs, int Ny, int Nz, int logn, double scale, int pitch = 0) {
    extern __shared__ double2 zbuf[];                 // [Nz][ZL]
    const int il = threadIdx.x % ZL, kq = threadIdx.x / ZL;       // 32 k-rows per pass
    const int i0 = blockIdx.x * ZL, j = blockIdx.y;
    const int i = i0 + il;
    const bool live = i < Nxs;
    const int ldx = pitch > 0 ? pitch : Nxs;          // row pitch of the spectrum (>= Nxs: padded to whole 128-B rows on the split path)
    const long plane = (long)ldx * Ny, base = (long)i + (long)ldx * j;
    if constexpr (NC > 0) {
        using LF = LineFFT<ZL, NC>;
        constexpr int KQ = LF::KQ, E = LF::E, LOGN = LF::LOGN;
        double2 r[E];
        LF::load(hc + ((long)(live ? i : i0) + (long)ldx * j) + plane * kq, plane, r);
        typename LF::Tw2 t2;
        typename LF::Tw4 t4;
        LF::dif_first_tw(tw, kq, t2, t4);
#pragma unroll
        for (int e = 0; e < E; ++e) zbuf[(kq + e * KQ) * ZL + il] = live ? r[e] : make_double2(0.0, 0.0);
        __syncthreads();
        // The last forward stage (span 2), the divide and the first inverse stage (span 1) of a thread work on the same four consecutive
        // points 4q .. 4q + 3: they stay in registers in between -- two LDS round trips and two barriers fewer than stage by stage, the
        // same operations on the same values. The eigenvalues of the divide and the twiddles of the two inverse stages that follow are
        // on their way while the forward stage before runs.
        static_assert(LF::NS4 >= 2, "the fused middle stages need two radix-4 stages");
        constexpr int I4 = LF::I4, QUARTER = LF::QUARTER;
        double lam[I4][4], lxy = 0.0;
        typename LF::Tw4 ti0, ti1;
        LF::template forward_to<LF::NS4 - 1>(zbuf, tw, il, kq, t2, t4, [&] {
            lxy = lx[live ? i : i0] + ly[j];
#pragma unroll
            for (int it = 0; it < I4; ++it)
#pragma unroll
                for (int m = 0; m < 4; ++m) lam[it][m] = lz[(int)(__brev((unsigned)(4 * (kq + it * KQ) + m) & (unsigned)(NC - 1)) >> (32 - LOGN))];
            LF::dit_tw4(tw, kq, 0, ti0);
            LF::dit_tw4(tw, kq, 1, ti1);
        });
#pragma unroll
        for (int it = 0; it < I4; ++it) {
            const int q = kq + it * KQ;
            if (QUARTER % KQ == 0 || q < QUARTER) {
                const int a = q << 2;
                double2 x[4] = {zbuf[a * ZL + il], zbuf[(a + 1) * ZL + il], zbuf[(a + 2) * ZL + il], zbuf[(a + 3) * ZL + il]};
                dif_butterfly4(x, t4.a[it], t4.b[it], t4.c[it]);
                if (live) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int k = (int)(__brev((unsigned)(a + m)) >> (32 - LOGN));
                        const double l = lxy + lam[it][m] - 0.0;
                        x[m].x = -(x[m].x * scale) / l;
                        x[m].y = -(x[m].y * scale) / l;
                        if (i == 0 && j == 0 && k == 0) x[m] = make_double2(0.0, 0.0);
                    }
                }
                dit_butterfly4(x, ti0.a[it], ti0.b[it], ti0.c[it]);
#pragma unroll
                for (int m = 0; m < 4; ++m) zbuf[(a + m) * ZL + il] = x[m];
            }
        }
        __syncthreads();
        LF::template inverse<1>(zbuf, tw, il, kq, ti1);
        if (live) {
#pragma unroll
            for (int e = 0; e < E; ++e) r[e] = zbuf[(kq + e * KQ) * ZL + il];
#pragma unroll
            for (int e = 0; e < E; ++e) hc[base + plane * (kq + e * KQ)] = r[e];
        }
        return;
    }
    const int KQ = 256 / ZL;
    const InterleavedLines<ZL> lines{zbuf, il, kq};
    for (int k = kq; k < Nz; k += KQ) zbuf[k * ZL + il] = live ? hc[base + plane * k] : make_double2(0.0, 0.0);
    __syncthreads();
    lds_fft_forward(lines, tw, Nz, logn);
    // spectral divide in bit-reversed order
    if (live) {
        const double lxy = lx[i] + ly[j];
        for (int p = kq; p < Nz; p += KQ) {
            const int k = (int)(__brev((unsigned)p) >> (32 - logn));
            double2 v = zbuf[p * ZL + il];
            const double lam = lxy + lz[k] - 0.0;
            v.x = -(v.x * scale) / lam;
            v.y = -(v.y * scale) / lam;
            if (i == 0 && j == 0 && k == 0) v = make_double2(0.0, 0.0);
            zbuf[p * ZL + il] = v;
        }
    }
    __syncthreads();
    lds_fft_inverse(lines, tw, Nz, logn);
    if (live)
        for (int k = kq; k < Nz; k += KQ) hc[base + plane * k] = zbuf[k * ZL + il];
}

// One-directional FFT of length N = 2^logn along the SLOWEST dimension of a (C, N) complex array (element (c, n) at c + C*n): the
// column transform rocFFT runs with its row kernel when it is planned as a 1-D strided transform (measured 129 us for 67 MB; this
// kernel: the same LDS machinery as zline_solve_kernel, ZL consecutive lines per workgroup: 8 = 128-B rows; 4 for lines of 512 and more,
// whose 64 KB of LDS per 8 lines leave two workgroups per CU -- measured at 512^3: 54.0 -> 51.9 ms/step with 4, 54.1 with 2; at 256^3 8 wins).
// forward: natural -> radix-4 DIF -> stored through the bit-reversal; inverse: loaded through the bit-reversal -> DIT -> natural,
// times `scale`. Same arithmetic as rocFFT's to round-off, not bitwise.
// NC > 0: N = NC at compile time (LineFFT above); NC = 0: any N = 2^logn, the generic loops.
template <int ZL, int NC = 0>
__global__ void __launch_bounds__(256, line_min_waves(ZL, NC)) strided_line_fft_kernel(double2 *data, const double2 *tw, long C, int N, int logn, int inverse,
                                                               double scale, long plane_stride = 0) {
    extern __shared__ double2 zbuf[];                 // [N][ZL]
    data += plane_stride * blockIdx.y;                // gridDim.y independent (C, N) arrays `plane_stride` elements apart
    const int il = threadIdx.x % ZL, kq = threadIdx.x / ZL;
    const long c = (long)blockIdx.x * ZL + il;
    const bool live = c < C;
    if constexpr (NC > 0) {
        using LF = LineFFT<ZL, NC>;
        constexpr int KQ = LF::KQ, E = LF::E, LOGN = LF::LOGN;
        double2 r[E];
        LF::load(data + (live ? c : (long)blockIdx.x * ZL) + C * kq, C, r);
        typename LF::Tw2 t2;
        typename LF::Tw4 t4;
        if (!inverse) {
            LF::dif_first_tw(tw, kq, t2, t4);
#pragma unroll
            for (int e = 0; e < E; ++e) zbuf[(kq + e * KQ) * ZL + il] = live ? r[e] : make_double2(0.0, 0.0);
            __syncthreads();
            LF::forward(zbuf, tw, il, kq, t2, t4);
            if (live) {
#pragma unroll
                for (int e = 0; e < E; ++e) r[e] = zbuf[(kq + e * KQ) * ZL + il];
#pragma unroll
                for (int e = 0; e < E; ++e) data[c + C * (long)(__brev((unsigned)(kq + e * KQ)) >> (32 - LOGN))] = r[e];
            }
        } else {
            LF::dit_tw4(tw, kq, 0, t4);
#pragma unroll
            for (int e = 0; e < E; ++e)
                zbuf[(int)(__brev((unsigned)(kq + e * KQ)) >> (32 - LOGN)) * ZL + il] = live ? r[e] : make_double2(0.0, 0.0);
            __syncthreads();
            LF::template inverse<0>(zbuf, tw, il, kq, t4);
            if (live) {
#pragma unroll
                for (int e = 0; e < E; ++e) r[e] = zbuf[(kq + e * KQ) * ZL + il];
#pragma unroll
                for (int e = 0; e < E; ++e) data[c + C * (kq + e * KQ)] = make_double2(r[e].x * scale, r[e].y * scale);
            }
        }
        return;
    }
    const int KQ = 256 / ZL;
    const InterleavedLines<ZL> lines{zbuf, il, kq};
    if (!inverse) {
        for (int k = kq; k < N; k += KQ) zbuf[k * ZL + il] = live ? data[c + C * k] : make_double2(0.0, 0.0);
        __syncthreads();
        lds_fft_forward(lines, tw, N, logn);
        if (live)
            for (int p = kq; p < N; p += KQ) data[c + C * (long)(__brev((unsigned)p) >> (32 - logn))] = zbuf[p * ZL + il];
    } else {
        for (int k = kq; k < N; k += KQ)
            zbuf[(int)(__brev((unsigned)k) >> (32 - logn)) * ZL + il] = live ? data[c + C * k] : make_double2(0.0, 0.0);
        __syncthreads();
        lds_fft_inverse(lines, tw, N, logn);
        if (live)
            for (int k = kq; k < N; k += KQ) {
                const double2 v = zbuf[k * ZL + il];
                data[c + C * k] = make_double2(v.x * scale, v.y * scale);
            }
    }
}

// The x stage of the distributed FFT solve in ONE pass (distributed_fft_based_poisson_solver.jl:152-166 with the transposes'
// unpack / pack folded in): a workgroup gathers L whole x-lines (length Nxg = R * Nxl, a power of two) from the all-to-all
// receive buffer -- chunk p holds columns [p*Nxl, (p+1)*Nxl) of every line (il fastest) --, transforms them forward (radix-4
// DIF), divides by the eigenvalues in bit-reversed order, transforms back (DIT) and scatters them into the send buffer in
// the same chunk layout. Replaces unpack + rocFFT + divide + rocFFT + pack (5 passes). LDS: L * Nxg complex.
__global__ void __launch_bounds__(256) xline_solve_kernel(const double2 *recv, double2 *send, const double2 *tw, const double *lx,
                                                          const double *ly, const double *lz, int R, int Nxl, int Nyc, int Nz,
                                                          int logn, int L, int joff, int Ny, double scale) {
    extern __shared__ double2 zbuf[];                 // [L][Nxg]
    const int N = R * Nxl;
    const long nlines = (long)Nyc * Nz, line0 = (long)blockIdx.x * L;
    const long chunk = (long)Nxl * nlines;
    const int total = L * N;
    const ContiguousLines lines{zbuf, L, logn};
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ln = e >> logn, n = e & (N - 1);
        const long line = line0 + ln;
        const int pch = n / Nxl, il = n - pch * Nxl;
        zbuf[e] = line < nlines ? recv[pch * chunk + il + (long)Nxl * line] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    lds_fft_forward(lines, tw, N, logn);
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ln = e >> logn, pz = e & (N - 1);
        const long line = line0 + ln;
        if (line >= nlines) continue;
        const int jl = (int)(line % Nyc), k = (int)(line / Nyc);
        const int i = (int)(__brev((unsigned)pz) >> (32 - logn));
        const int jg = min(joff + jl, Ny - 1);
        double2 v = zbuf[e];
        const double lam = (lx[i] + ly[jg]) + lz[k] - 0.0;
        v.x = -(v.x * scale) / lam;
        v.y = -(v.y * scale) / lam;
        if (i == 0 && joff + jl == 0 && k == 0) v = make_double2(0.0, 0.0);
        zbuf[e] = v;
    }
    __syncthreads();
    lds_fft_inverse(lines, tw, N, logn);
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ln = e >> logn, n = e & (N - 1);
        const long line = line0 + ln;
        if (line >= nlines) continue;
        const int pch = n / Nxl, il = n - pch * Nxl;
        send[pch * chunk + il + (long)Nxl * line] = zbuf[e];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The z transform of the x-fastest substructured solve (ocn_kernels.h "xfast"): the real-to-complex transform of TWO neighbouring x
// columns at once -- (r[2i'], r[2i'+1]) read as one complex number, a complex line FFT along z in LDS, and the two columns' half spectra
// separated with the Hermitian symmetry WHILE THE LINE IS IN LDS.
// ---------------------------------------------------------------------------------------------------------------------
// Hermitian separation of the transformed pair line il of zbuf[N][ZL] (bit-reversed order) into spec[2c + 2C kz], spec[2c + 1 + 2C kz],
// kz = 0 .. N/2: with Z = FFT(r_even + i r_odd), X_even[k] = (Z[k] + conj Z[N-k]) / 2, X_odd[k] = (Z[k] - conj Z[N-k]) / (2i)
template <int ZL>
__device__ __forceinline__ void paired_zline_separate(const double2 *zbuf, double2 *spec, long c, long C, int N, int logn, int il, int kq) {
    for (int kz = kq; kz <= (N >> 1); kz += 256 / ZL) {
        const int pa = (int)(__brev((unsigned)kz) >> (32 - logn)), pb = (int)(__brev((unsigned)((N - kz) & (N - 1))) >> (32 - logn));
        const double2 a = zbuf[pa * ZL + il], b = zbuf[pb * ZL + il];
        double2 *o = spec + 2 * c + 2 * C * (long)kz;
        o[0] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
        o[1] = make_double2(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));
    }
}
// real-to-complex along z of the column PAIRS of a dense x-fastest real array: rp[c + C k] = (r[2c], r[2c+1]) at level k, c = pair index
// over (x, y) (C = Nx Ny / 2 pairs per level); out: the half spectra of the two columns (paired_zline_separate)
template <int ZL>
__global__ void __launch_bounds__(256) paired_zline_r2c_kernel(const double2 *rp, double2 *spec, const double2 *tw, long C, int N, int logn) {
    extern __shared__ double2 zbuf[];                 // [N][ZL]
    const int il = threadIdx.x % ZL, kq = threadIdx.x / ZL, KQ = 256 / ZL;
    const long c = (long)blockIdx.x * ZL + il;
    const bool live = c < C;
    for (int k = kq; k < N; k += KQ) zbuf[k * ZL + il] = live ? rp[c + C * k] : make_double2(0.0, 0.0);
    __syncthreads();
    lds_fft_forward(InterleavedLines<ZL>{zbuf, il, kq}, tw, N, logn);
    if (!live) return;
    paired_zline_separate<ZL>(zbuf, spec, c, C, N, logn, il, kq);
}
// the way back: Z[k] = X_even[k] + i X_odd[k], Z[N-k] = conj X_even[k] + i conj X_odd[k]; the imaginary parts of the k = 0 and k = N/2
// entries are ignored like a complex-to-real transform ignores them; rp = Re / Im of the inverse transform, times `scale`
template <int ZL>
__global__ void __launch_bounds__(256) paired_zline_c2r_kernel(const double2 *spec, double2 *rp, const double2 *tw, long C, int N, int logn, double scale) {
    extern __shared__ double2 zbuf[];
    const int il = threadIdx.x % ZL, kq = threadIdx.x / ZL, KQ = 256 / ZL;
    const long c = (long)blockIdx.x * ZL + il;
    const bool live = c < C;
    for (int kz = kq; kz <= (N >> 1); kz += KQ) {
        const double2 *in = spec + 2 * c + 2 * C * (long)kz;
        const double2 E = live ? in[0] : make_double2(0.0, 0.0), O = live ? in[1] : make_double2(0.0, 0.0);
        const int pa = (int)(__brev((unsigned)kz) >> (32 - logn));
        if (kz == 0 || kz == (N >> 1)) zbuf[pa * ZL + il] = make_double2(E.x, O.x);
        else {
            const int pb = (int)(__brev((unsigned)(N - kz)) >> (32 - logn));
            zbuf[pa * ZL + il] = make_double2(E.x - O.y, E.y + O.x);
            zbuf[pb * ZL + il] = make_double2(E.x + O.y, O.x - E.y);
        }
    }
    __syncthreads();
    lds_fft_inverse(InterleavedLines<ZL>{zbuf, il, kq}, tw, N, logn);
    if (!live) return;
    for (int k = kq; k < N; k += KQ) {
        const double2 v = zbuf[k * ZL + il];
        rp[c + C * k] = make_double2(v.x * scale, v.y * scale);
    }
}
