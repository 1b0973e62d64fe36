// k_multi.hip -- the multi-vector apply (mas_apply_multi_device): one prepared
// handle applied to K residuals in one pass over the inverses.
//
// The apply is bound by bytes, and almost all of them are the level-0 inverses
// (k_apply.hip): 14 272 B per 32-vertex block against 48 B per vertex of map,
// r and z.  The inverses do not depend on the residual, so every kernel here
// loads a block's inverse once and solves it for K vectors:
//   k_coarse_l1_multi   level 1: the block's inverse and the 32 l1src ids per
//                       node once; per vector the children's r gathered and
//                       folded in lane order from +0 (as k_coarse_l1; the two
//                       halves of the wave take a vector each), the K solves
//                       interleaved, R1_k / Z1_k stored
//   k_coarse_up_multi   levels 2 and (grouped) 3 the same way from members
//   k_solve_fine_multi  level 0: map and record once (the 24-bit copy decoded
//                       once); per vector gather, solve, prolongation, scatter
// One launch per level, ordered by the stream alone: no device-side wait, no
// host epoch (the tagged one-launch form k_coarse1.hip is not used here), so
// nothing can time out and a captured graph replays it as it is.  With
// reference_restriction at L >= 4 level 3 runs k_coarse_deep once per vector.
//
// Bitwise contract: z_k is bit for bit what run_apply writes for r_k.  Every
// FMA / add is an explicit intrinsic (-ffp-contract=off), the per-vector
// operation order is block_solve's (pair_step is shared) and the folds are the
// per-level form's, which is bitwise equal to the other coarse forms.
//
// Coarse R / Z of vector k live in slab k of RcMulti / ZcMulti (the coarse node
// range each); the single-vector Rc / Zc are not touched.  Batches of more
// than kMultiK vectors run as ceil(count / kMultiK) passes of near-equal size
// (5 = 3 + 2, 8 = 4 + 4), each over its own slabs.
#include "block_solve.h"

namespace mas {

constexpr int kMultiK = 4;  // vectors per pass: the largest templated K

// the vectors of one pass, by value in the kernel arguments (no device-side table)
struct MultiVecs {
    const float4* r[kMultiK];
    float4* z[kMultiK];
};

// x, y, z of a float4 vector entry as one 12-byte load: w is never read, and a
// batch keeps K times as many gathered values in registers as a single apply
__device__ __forceinline__ float3 load_xyz(const float4* p) {
    typedef float v3f __attribute__((ext_vector_type(3)));
    const v3f t = *reinterpret_cast<const v3f*>(p);
    return make_float3(t.x, t.y, t.z);
}

// out[k] = Inv_b r[k]: block_solve (block_solve.h) for K vectors, the K solves
// interleaved inside each rotation step so that the step's G registers are
// shared and the shuffles of one vector overlap the FMAs of another.  Per
// vector the operations and their order are exactly block_solve's.
template <int K>
__device__ __forceinline__ void block_solve_multi(const float (&g)[kRecord], const float (&tl)[3],
                                                  const float3 (&r)[K], int lane, float3 (&out)[K]) {
    const int n = lane & 31, hb = lane & 32;
    const bool h1 = hb != 0;
#pragma unroll
    for (int v = 0; v < K; ++v) {  // D(n) r, half 0 only
        const float ox = __fmaf_rn(g[68], r[v].z, __fmaf_rn(g[67], r[v].y, __fmul_rn(g[66], r[v].x)));
        const float oy = __fmaf_rn(g[70], r[v].z, __fmaf_rn(g[69], r[v].y, __fmul_rn(g[67], r[v].x)));
        const float oz = __fmaf_rn(g[71], r[v].z, __fmaf_rn(g[70], r[v].y, __fmul_rn(g[68], r[v].x)));
        out[v] = h1 ? make_float3(0.f, 0.f, 0.f) : make_float3(ox, oy, oz);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int s = h1 ? 8 + k : 1 + k;
        float G[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) G[e] = g[9 * k + e];
#pragma unroll
        for (int v = 0; v < K; ++v) pair_step(out[v], G, r[v], hb | ((n + s) & 31), hb | ((n - s) & 31));
    }
    {  // k = 7: half 1 regular s = 15; half 0 the s = 16 pair (block_solve)
        const bool lo = n < 16;
        const float w0 = g[63], w1 = g[64], w2 = g[65];
        // the same values as block_solve's, by selects alone: behind a branch
        // here the compiler sinks every vector's accumulation chain below it, and
        // the shuffle results of all eight steps stay live (K x 48 registers)
        float G0[9];
        G0[0] = lo ? w0 : 0.f;  G0[1] = lo ? w1 : w0;   G0[2] = lo ? w2 : 0.f;
        G0[3] = 0.f;            G0[4] = lo ? 0.f : w1;  G0[5] = 0.f;
        G0[6] = lo ? tl[0] : 0.f; G0[7] = lo ? tl[1] : w2; G0[8] = lo ? tl[2] : 0.f;
        float G[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) G[e] = h1 ? g[63 + e] : G0[e];
        const int s = h1 ? 15 : 16;
#pragma unroll
        for (int v = 0; v < K; ++v) pair_step(out[v], G, r[v], hb | ((n + s) & 31), hb | ((n - s) & 31));
    }
    const int other = lane ^ 32;
#pragma unroll
    for (int v = 0; v < K; ++v) {
        out[v].x = __fadd_rn(out[v].x, __shfl(out[v].x, other));
        out[v].y = __fadd_rn(out[v].y, __shfl(out[v].y, other));
        out[v].z = __fadd_rn(out[v].z, __shfl(out[v].z, other));
    }
}

// Level 0 (solve_fine_body of k_apply.hip for K vectors): one wave per block in
// two-wave workgroups numbered in XCD chunks.  zc: slab 0 of the pass's coarse
// Z, slab k at zc + k * slab.  NT: nontemporal inverse loads (fine_var).
template <int NPROL, int K, bool NARROW, bool NT>
__global__ __launch_bounds__(128) void k_solve_fine_multi(const void* __restrict__ inv, int nFineBlk, int nV,
                                                         MultiVecs vec, const int4* __restrict__ vmap,
                                                         const float4* __restrict__ zc, int slab, int begin1) {
    const int lane = threadIdx.x & 63, n = lane & 31;
    const int blk = xcd_chunked(blockIdx.x, gridDim.x) * 2 + (threadIdx.x >> 6);
    const bool bvalid = blk < nFineBlk;
    const int v = blk * 32 + n;
    const bool vvalid = bvalid && v < nV;
    const int4 m = vmap[vvalid ? v : 0];
    float g[kRecord], tl[3];
    if (NARROW) load_record_narrow<NT>(inv, bvalid ? blk : 0, lane, g, tl);
    else load_record<NT>(static_cast<const float4*>(inv), bvalid ? blk : 0, lane, g, tl);
    float3 rr[K], out[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float3 rv = load_xyz(vec.r[k] + m.x);
        rr[k] = vvalid ? rv : make_float3(0.f, 0.f, 0.f);
    }
    block_solve_multi<K>(g, tl, rr, lane, out);
    if (!(vvalid && lane < 32)) return;
    // every coarse Z before the first store: z_k may not alias them, but the
    // compiler cannot know that of pointers passed by value
    float3 a1[K], a2[K], a3[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float4* zk = zc + (size_t)k * slab;
        if (NPROL >= 1) a1[k] = load_xyz(zk + (m.y - begin1));
        if (NPROL >= 2) a2[k] = load_xyz(zk + (m.z - begin1));
        if (NPROL >= 3) a3[k] = load_xyz(zk + (m.w - begin1));
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {  // CollectFinalZ order
        float3 o = out[k];
        if (NPROL >= 1) {
            o.x = __fadd_rn(o.x, a1[k].x); o.y = __fadd_rn(o.y, a1[k].y); o.z = __fadd_rn(o.z, a1[k].z);
        }
        if (NPROL >= 2) {
            o.x = __fadd_rn(o.x, a2[k].x); o.y = __fadd_rn(o.y, a2[k].y); o.z = __fadd_rn(o.z, a2[k].z);
        }
        if (NPROL >= 3) {
            o.x = __fadd_rn(o.x, a3[k].x); o.y = __fadd_rn(o.y, a3[k].y); o.z = __fadd_rn(o.z, a3[k].z);
        }
        vec.z[k][m.x] = make_float4(o.x, o.y, o.z, 0.f);
    }
}

// One coarse block for K vectors (coarse_block_l1 / coarse_block_up and
// coarse_finish of k_apply.hip).  has(j): lane j of the child bank is a child
// of this lane's node n (the same answer in both halves of the wave);
// base(k) + off(j): the address of that child's value for vector k.
//
// The two halves of the wave share the gathers: for each pair of vectors half 0
// gathers and folds node n's children for the first and half 1 for the second
// -- per vector the children in lane order from +0, as the single-vector kernels
// fold them -- so a lane holds 32 values per PAIR and every pair's gathers are
// in flight together (K x 32 values per lane in half 0 alone did not fit the
// register file).  A shuffle then hands each vector's R to both halves, the K
// solves run interleaved, and R_k / Z_k go to the vectors' slabs.
template <int K, class Has, class Base, class Off>
__device__ __forceinline__ void coarse_block_multi(const float (&g)[kRecord], const float (&tl)[3], int lane, int n,
                                                   int node, Has has, Base base, Off off, float4* __restrict__ rc,
                                                   float4* __restrict__ zc, int slab, int begin1) {
    constexpr int kPairs = (K + 1) / 2;
    const bool h1 = lane >= 32;
    float vx[kPairs][32], vy[kPairs][32], vz[kPairs][32];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        const bool second = 2 * p + 1 < K;  // an odd K leaves half 1 idle in the last pair
        const float4* b = h1 ? base(second ? 2 * p + 1 : 2 * p) : base(2 * p);
        const bool act = !h1 || second;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            float3 t = make_float3(0.f, 0.f, 0.f);
            if (act && has(j)) t = load_xyz(b + off(j));
            vx[p][j] = t.x;
            vy[p][j] = t.y;
            vz[p][j] = t.z;
        }
    }
    float3 a[K], out[K];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (has(j)) {
                ax = __fadd_rn(ax, vx[p][j]);
                ay = __fadd_rn(ay, vy[p][j]);
                az = __fadd_rn(az, vz[p][j]);
            }
        }
        // node n's R of the pair's first vector from lane n, of its second from lane 32 + n
        a[2 * p] = make_float3(__shfl(ax, n), __shfl(ay, n), __shfl(az, n));
        if (2 * p + 1 < K) a[2 * p + 1] = make_float3(__shfl(ax, 32 + n), __shfl(ay, 32 + n), __shfl(az, 32 + n));
    }
    block_solve_multi<K>(g, tl, a, lane, out);
    if (lane < 32) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rc[(size_t)k * slab + node - begin1] = make_float4(a[k].x, a[k].y, a[k].z, 0.f);
            zc[(size_t)k * slab + node - begin1] = make_float4(out[k].x, out[k].y, out[k].z, 0.f);
        }
    }
}

// Level 1, one wave per block: the children's original vertex ids from l1src
// (32 per node, -1 where the lane is not a child), loaded once for the K vectors.
template <int K>
__global__ __launch_bounds__(kApplyThreads) void k_coarse_l1_multi(const float4* __restrict__ inv, int blkBegin,
                                                                  int nb, int count,
                                                                  const int* __restrict__ l1src, MultiVecs vec,
                                                                  float4* __restrict__ rc, float4* __restrict__ zc,
                                                                  int slab, int begin1) {
    const int w = blockIdx.x * (kApplyThreads / 64) + (threadIdx.x >> 6);
    if (w >= nb) return;  // wave-uniform
    const int lane = threadIdx.x & 63, n = lane & 31;
    const int blk = blkBegin + w, node = blk * 32 + n;
    float g[kRecord], tl[3];
    load_record<true>(inv, blk, lane, g, tl);
    const bool own = (node - blkBegin * 32) < count;  // both halves: lane 32 + n gathers for node n too
    int src[32];
    const int4* s4 = reinterpret_cast<const int4*>(l1src + (size_t)(node - blkBegin * 32) * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int4 t = own ? s4[q] : make_int4(-1, -1, -1, -1);
        src[4 * q + 0] = t.x;
        src[4 * q + 1] = t.y;
        src[4 * q + 2] = t.z;
        src[4 * q + 3] = t.w;
    }
    coarse_block_multi<K>(
        g, tl, lane, n, node, [&](int j) { return src[j] >= 0; }, [&](int k) { return vec.r[k]; },
        [&](int j) { return src[j]; }, rc, zc, slab, begin1);
}

// Levels >= 2: the children are the lanes `mask` of child bank `bank`
// (members, loaded once), their R in the vector's own slab.
template <int K>
__global__ __launch_bounds__(kApplyThreads) void k_coarse_up_multi(const float4* __restrict__ inv, int blkBegin,
                                                                  int nb, int count,
                                                                  const int2* __restrict__ members, int childBegin,
                                                                  float4* __restrict__ rc, float4* __restrict__ zc,
                                                                  int slab, int begin1) {
    const int w = blockIdx.x * (kApplyThreads / 64) + (threadIdx.x >> 6);
    if (w >= nb) return;  // wave-uniform
    const int lane = threadIdx.x & 63, n = lane & 31;
    const int blk = blkBegin + w, node = blk * 32 + n;
    float g[kRecord], tl[3];
    load_record<true>(inv, blk, lane, g, tl);
    const bool own = (node - blkBegin * 32) < count;  // both halves, as level 1
    const int2 mb = own ? members[node - begin1] : make_int2(0, 0);
    const unsigned msk = (unsigned)mb.y;
    const int cbase = childBegin + mb.x * 32 - begin1;
    const float4* rcc = rc;
    coarse_block_multi<K>(
        g, tl, lane, n, node, [&](int j) { return ((msk >> j) & 1u) != 0; },
        [&](int k) { return rcc + ((size_t)k * slab + cbase); }, [&](int j) { return j; }, rc, zc, slab, begin1);
}

template <int NPROL, int K>
static void launch_fine_multi(mas_context* h, const MultiVecs& vec, const float4* zc, int slab, hipStream_t s) {
    const int nb = h->nFineBlk, nV = h->nV, begin1 = h->levelSize[3];
    const int var = fine_var(h, nb, K);
    // the copy and the cache policy the single-vector launch of this handle takes (launch_fine_n)
    const void* invN = (var == 6 || var == 8) ? narrow_inv(h) : nullptr;
    const bool nt = var != 0 && var != 8;
    const int4* vmap = P<int4>(h->vmap);
    const dim3 grid(cdiv(nb, 2)), block(128);
    if (invN) {
        if (nt) k_solve_fine_multi<NPROL, K, true, true><<<grid, block, 0, s>>>(invN, nb, nV, vec, vmap, zc, slab, begin1);
        else k_solve_fine_multi<NPROL, K, true, false><<<grid, block, 0, s>>>(invN, nb, nV, vec, vmap, zc, slab, begin1);
    } else {
        const void* inv = h->inv.p;
        if (nt) k_solve_fine_multi<NPROL, K, false, true><<<grid, block, 0, s>>>(inv, nb, nV, vec, vmap, zc, slab, begin1);
        else k_solve_fine_multi<NPROL, K, false, false><<<grid, block, 0, s>>>(inv, nb, nV, vec, vmap, zc, slab, begin1);
    }
}

// one pass: K vectors, their coarse slabs starting at rc / zc
template <int K>
static void launch_pass(mas_context* h, const MultiVecs& vec, float4* rc, float4* zc, int slab, hipStream_t s) {
    const int L = h->L, begin1 = h->levelSize[3];
    const float4* inv = P<float4>(h->inv);
    // grouped level 3 (the default): one more `up` launch; else the reference's fold over R1, per vector
    const int lTop = h->groupedR3 ? 4 : 3;
    const int wpb = kApplyThreads / 64;
    for (int l = 1; l < L && l < lTop; ++l) {
        const int cnt = h->levelSize[2 * l], beg = h->levelSize[2 * l + 1];
        const int nb = ceil32(cnt) / 32;
        if (l == 1)
            k_coarse_l1_multi<K><<<cdiv(nb, wpb), kApplyThreads, 0, s>>>(inv, beg / 32, nb, cnt, P<int>(h->l1src), vec,
                                                                         rc, zc, slab, begin1);
        else
            k_coarse_up_multi<K><<<cdiv(nb, wpb), kApplyThreads, 0, s>>>(inv, beg / 32, nb, cnt, P<int2>(h->members),
                                                                         h->levelSize[2 * (l - 1) + 1], rc, zc, slab,
                                                                         begin1);
    }
    if (L >= 4 && !h->groupedR3)
        for (int k = 0; k < K; ++k)
            launch_coarse_deep(h, nullptr, nullptr, s, rc + (size_t)k * slab, zc + (size_t)k * slab);
    switch (L < 4 ? L - 1 : 3) {
        case 0: launch_fine_multi<0, K>(h, vec, zc, slab, s); break;
        case 1: launch_fine_multi<1, K>(h, vec, zc, slab, s); break;
        case 2: launch_fine_multi<2, K>(h, vec, zc, slab, s); break;
        default: launch_fine_multi<3, K>(h, vec, zc, slab, s); break;
    }
}

int run_apply_multi(mas_context* h, int count, float4* const* d_z, const float4* const* d_r, hipStream_t s) {
    if (count < 2 || count > MAS_MAX_RHS) return fail(h, MAS_ERR_ARG, "apply (multi): 2 .. MAS_MAX_RHS vectors");
    if (h->L >= 4 && !h->deepOff.p) return fail(h, MAS_ERR_STATE, "apply: deep-level lists not built");
    if (h->fineBlk0 != 0 || h->fineBlk1 != h->nFineBlk)
        return fail(h, MAS_ERR_STATE, "apply: the handle was prepared for one shard (mas_set_prepare_shard); "
                                      "use the sharded apply of that shard");
    // slab k: the coarse node range of vector k
    const int nCoarse = h->L > 1 ? h->totalClusters - h->levelSize[3] : 0;
    const size_t need = (size_t)count * nCoarse * sizeof(float4);
    if (need > h->RcMulti.bytes || need > h->ZcMulti.bytes) {
        // an earlier batch may still read the slabs about to be freed, on any
        // stream (this fails inside a stream capture: mas_capi.h)
        int rc = hip_check(h, hipDeviceSynchronize(), "apply (multi): growing the coarse slabs");
        if (rc || (rc = ensure(h, h->RcMulti, need)) || (rc = ensure(h, h->ZcMulti, need))) return rc;
    }
    const int passes = cdiv(count, kMultiK);
    for (int p = 0, k0 = 0; p < passes; ++p) {
        const int K = count / passes + (p < count % passes ? 1 : 0);
        MultiVecs vec{};
        for (int k = 0; k < K; ++k) {
            vec.r[k] = d_r[k0 + k];
            vec.z[k] = d_z[k0 + k];
        }
        float4* rc = P<float4>(h->RcMulti) + (size_t)k0 * nCoarse;
        float4* zc = P<float4>(h->ZcMulti) + (size_t)k0 * nCoarse;
        switch (K) {
            case 2: launch_pass<2>(h, vec, rc, zc, nCoarse, s); break;
            case 3: launch_pass<3>(h, vec, rc, zc, nCoarse, s); break;
            default: launch_pass<4>(h, vec, rc, zc, nCoarse, s); break;
        }
        k0 += K;
    }
    h->stats.apply_calls += count;
    return hip_check(h, hipGetLastError(), "apply kernels (multi)");
}

}  // namespace mas
