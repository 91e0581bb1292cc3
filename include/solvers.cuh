// Solvers for N-body problems of spheroid cells on MI355X (gfx950).
//
// Source-level API parity with ya||a `include/solvers.cuh` (reference lines
// cited per item): Pairwise_interaction / Pairwise_friction / Generic_forces
// signatures and the default frictions (:15-50), Solution<Pt, Solver> (:56-106),
// Heun_solver with set_fixed* (:164-276), Tile_solver (:279-342), Grid with its
// four public arrays and d_grid mirror (:380-425), __constant__ d_nhood[27]
// (:428), Grid_solver with public cube_size (:465-502).
//
// The implementation is new and CDNA4-first; what differs from the reference:
//
//  * One fused force kernel per stage.  The reference runs 3 fills, the force
//    kernel, add_rhs, a thrust::reduce with a blocking device->host copy and the
//    update kernel (:231-255).  Here the force kernel writes
//    dX = gen + F + sum_v / sum_friction directly (no fills, no add_rhs, no
//    d_sum_v / d_sum_friction arrays), the centre-of-mass mean is reduced on the
//    device into a buffer the update kernel reads, and nothing but the 4-byte
//    read of n at step entry (:229) touches the host.
//  * Grid force: cells are processed in cube-sorted order from a gathered,
//    16-byte-aligned copy {X, id} (+ old_v) so neighbour reads are contiguous:
//    the 27 stencil cubes are 9 x-rows of 3 consecutive cube ids, i.e. 9
//    contiguous slot ranges of the sorted array; they are walked in exactly the
//    reference's d_nhood order (:472-483) and ascending point id inside a cube.
//    THE SUMMATION ORDER (round 5; every grid kernel and the oracle): a cell's
//    terms from its own z-plane (d_nhood[0..8]) and those from the planes below
//    and above ([9..26]) are summed separately, each in that order from +0, and
//    the two sums are added -- where the reference's thread adds all 27 cubes'
//    terms to one sum (:437-459).  It lets grid_force_bits give a tile's planes
//    to two wavefronts where that shortens a launch ("the tail"); ~1e-7 relative
//    per step beside the reference's association.
//  * Tile force: 64-thread (one wavefront) workgroups, 256-point LDS tiles
//    holding X and old_v, two barriers per tile (the reference's single barrier
//    at :302 is only safe for a 32-thread block on a 32-wide warp).
//  * One thread owns one cell i for the whole stage, as in the reference:
//    functors may update per-i state non-atomically
//    (examples/passive_growth.cu:48-51) and see original point ids.
//
// Arithmetic contract: pair distance is sqrtf(fmaf(z,z,fmaf(y,y,x*x))); all
// other arithmetic is the reference's statement-by-statement binary32.  Build
// model files with -ffp-contract=off to reproduce the CPU oracle bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "cudebug.cuh"
#include "dtypes.cuh"
#include "fold256.cuh"
#include "grid_bin.cuh"
#include "yalla_hip.h"

// Model files use thrust::fill / reduce on their own arrays and rely on the
// reference's solvers.cuh for the includes (examples/branching.cu:189).  The
// engine itself does not use Thrust; define YALLA_NO_THRUST to skip them.
#ifndef YALLA_NO_THRUST
#include <thrust/execution_policy.h>
#include <thrust/fill.h>
#include <thrust/reduce.h>
#include <thrust/sort.h>
#endif


// Interactions are specified between two points Xi and Xj with r = Xi - Xj
// (solvers.cuh:15-19).
template<typename Pt>
using Pairwise_interaction = Pt(Pt Xi, Pt r, float dist, int i, int j);

// Pairwise friction coefficient (solvers.cuh:21-41).
template<typename Pt>
using Pairwise_friction = float(Pt Xi, Pt r, float dist, int i, int j);

template<typename Pt>
__device__ float friction_w_neighbour(Pt Xi, Pt r, float dist, int i, int j)
{
    if (i == j) return 0;
    return dist < 1 ? 1 : 0;
}

template<typename Pt>
__device__ float friction_on_background(Pt Xi, Pt r, float dist, int i, int j)
{
    return 0;
}

// Optional generic forces, run before the pairwise interactions
// (solvers.cuh:43-53).
template<typename Pt>
using Generic_forces =
    std::function<void(const int n, const Pt* __restrict__ d_X, Pt* d_dX)>;

template<typename Pt>
void no_gen_forces(const int n, const Pt* __restrict__ d_X, Pt* d_dX)
{}


// ---- stateless functors ----------------------------------------------------------------------
// One thread owns one cell for a whole stage because a functor may keep per-cell state without
// atomics (`d_mes_nbs[i] += 1`, examples/passive_growth.cu:48-51).  Most functors do not: they are
// pure functions of their arguments, or count with atomicAdd (examples/branching.cu:105-107).
// A model says so with ONE line next to the functor,
//
//     __device__ float3 my_force(float3 Xi, float3 r, float dist, int i, int j) { ... }
//     YA_STATELESS(float3, my_force)
//
// and the solvers then pick the kernels that share a cell among several lanes whenever the
// system is too small to fill the chip with one lane per cell (ya::tile_force_coop,
// ya::grid_force_coop: 2-8 x faster steps below ~10^5 cells, bit-identical results: every sum is
// still accumulated in the one-lane kernels' order) and split the last tiles of large launches between two
// wavefronts (grid_force_bits, "the tail").  Custom friction functors take
// YA_STATELESS_FRICTION; the two defaults are known to be stateless.
namespace ya {
template<typename Pt, Pairwise_interaction<Pt> pw_int>
struct Stateless_interaction : std::false_type {};
template<typename Pt, Pairwise_friction<Pt> pw_friction>
struct Stateless_friction : std::false_type {};
// the two default frictions, for any point type (compared as template arguments: class scope,
// where naming a __device__ function is allowed on the host side too)
template<typename Pt, Pairwise_friction<Pt> pw_friction>
struct Default_friction {
    static constexpr bool value =
        pw_friction == &friction_w_neighbour<Pt> || pw_friction == &friction_on_background<Pt>;
};
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
constexpr bool stateless_pair()
{
    return Stateless_interaction<Pt, pw_int>::value &&
           (Default_friction<Pt, pw_friction>::value || Stateless_friction<Pt, pw_friction>::value);
}
}  // namespace ya
#define YA_STATELESS(Pt_, functor_)                                            \
    namespace ya {                                                            \
    template<>                                                                \
    struct Stateless_interaction<Pt_, functor_> : std::true_type {};          \
    }
#define YA_STATELESS_FRICTION(Pt_, functor_)                                   \
    namespace ya {                                                            \
    template<>                                                                \
    struct Stateless_friction<Pt_, functor_> : std::true_type {};             \
    }


namespace ya {

#ifndef YA_FORCE_BLOCK
#define YA_FORCE_BLOCK 256
#endif
constexpr int FORCE_BLOCK = YA_FORCE_BLOCK;  // grid force: cells (threads) per workgroup
constexpr int TILE_BLOCK = 64;     // tile force: one wavefront per workgroup
constexpr int TILE_POINTS = 256;   // points staged in LDS per tile
constexpr int UPDATE_BLOCK = 256;
static_assert(UPDATE_BLOCK == 256, "the update kernels fold partial sums with ya::fold256, libyalla_hip.so's order");

// One cell in cube-sorted order: the point and its original id.  16-byte
// entries (float3) load as one dwordx4.
template<typename Pt>
struct alignas(alignof(Pt) > ((sizeof(Pt) + 4) % 16 == 0 ? 16 : ((sizeof(Pt) + 4) % 8 == 0 ? 8 : 4))
                   ? alignof(Pt)
                   : ((sizeof(Pt) + 4) % 16 == 0 ? 16 : ((sizeof(Pt) + 4) % 8 == 0 ? 8 : 4))) Entry {
    Pt X;
    int id;
};

// Correctly rounded square root for x = 0 or x >= 2^-96 (every squared distance
// between distinct binary32 positions of a model): the hardware estimate
// (v_sqrt_f32, <= 1 ulp) moved down or up by one ulp according to the sign of the
// exact residuals x - (s -+ 1ulp) * s, which is the core of the compiler's own
// expansion of sqrtf without its rescaling of tiny arguments (10 fewer VALU
// instructions per interacting pair).  Tiny non-zero arguments take the library
// path.  Verified against sqrtf for EVERY binary32 argument by
// tests/test_parity_gpu.py (ya::check_sqrt_all).
//
// YA_ARITH_FAST (a build switch for a model's translation unit, together with
// -ffp-contract=fast): the fast-arithmetic tier.  The pair distance is the bare v_sqrt_f32
// (<= 1 ulp, as CUDA's norm3df, which the reference calls at solvers.cuh:308,449), `Pt / float`
// multiplies by the bare v_rcp_f32 (<= 1 ulp), and multiply-adds are contracted as nvcc
// contracts them for the reference's CUDA build.  Results then agree with the exact tier (and
// the oracle) to rounding, i.e. far inside north_star's 1e-5 relative on positions
// (tests/test_fast_arith_gpu.py holds every configuration's functor to that in lock-step), but
// not bit for bit; cube ids, cell counts and the grid arrays stay bit-exact (they are computed in
// libyalla_hip.so, which is always built without contraction).  -18 % on the 1 M-cell force launch.
__device__ __forceinline__ float exact_sqrt(float x)
{
#ifdef YA_ARITH_FAST
    return __builtin_amdgcn_sqrtf(x);
#endif
    // The common path runs unconditionally; the rare one (a tiny non-zero argument)
    // replaces its result afterwards: one skipped branch per call instead of a two-sided one.
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_down = __int_as_float(__float_as_int(s) - 1);
    const float s_up = __int_as_float(__float_as_int(s) + 1);
    const float r_down = fmaf(-s_down, s, x);
    const float r_up = fmaf(-s_up, s, x);
    float out = r_down <= 0.f ? s_down : s;
    out = r_up > 0.f ? s_up : out;
    if (__builtin_expect(x < 0x1p-96f && x > 0.f, 0)) out = sqrtf(x);
    return out;
}

__device__ __forceinline__ float dist3(float x, float y, float z)
{
    return exact_sqrt(fmaf(z, z, fmaf(y, y, x * x)));
}

// Test hook: counts the binary32 bit patterns in [first, last] for which
// exact_sqrt differs from sqrtf (NaNs compare by class).
__global__ void check_sqrt_all(unsigned first, unsigned last, unsigned long long* mismatches)
{
    unsigned long long bad = 0;
    for (unsigned long long u = (unsigned long long)first + blockIdx.x * blockDim.x + threadIdx.x;
         u <= last; u += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __int_as_float((int)(unsigned)u);
        const float a = exact_sqrt(x), b = sqrtf(x);
        if (__float_as_int(a) != __float_as_int(b) && !(a != a && b != b)) bad++;
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Workgroup -> tile mapping that gives each of the 8 XCDs one contiguous range of
// tiles.  The dispatcher places block b on XCD b % 8 (MI355X_MICROARCH.md, workgroup
// dispatch): with the identity mapping every XCD's 4 MiB L2 sees the whole sorted
// array; with this one it sees an eighth of it, which is about what it can hold at
// 10^6 cells, so the stencil rows a tile reads (the tiles before and after it, one
// grid row and one grid plane away) are L2 hits.  Bijective for any grid size; a
// wrong placement guess would cost speed, not correctness.
__device__ __forceinline__ int xcd_eighth_tile(const int block, const int n_blocks, const bool descending = false)
{
    constexpr int XCDS = 8;
    const int xcd = block % XCDS, turn = block / XCDS;
    const int q = n_blocks / XCDS, r = n_blocks % XCDS;
    const int mine = q + (xcd < r ? 1 : 0);  // tiles of this XCD's eighth
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (descending ? mine - 1 - turn : turn);
}
// Each XCD gets TWO contiguous sixteenths: one from the lower half of the tiles and the
// corresponding one from the upper half.  Tiles are in cube order (z-major), and a tile's cost
// follows the local density of neighbours: for a ball of cells it rises from the first tiles
// (a polar cap: many surface cells) to the middle and falls again, so eighths in order leave
// the XCDs of the caps idle at the end of a launch while those of the equator still work.
// Pairing sixteenth k of the lower half with sixteenth k of the upper half evens that out and
// keeps an XCD's L2 to two contiguous ranges.
// Round 4, OUTSIDE IN: the ranges are visited alternately from the front and from the back of the
// list -- 0, R - 1, 1, R - 2, ... -- and those from the back are walked downwards.  The list's two
// ends are the tips of the ball's caps, where a plane of the grid holds a few hundred cells: a tile
// of 64 cells spans several grid rows there, its nine stencil rows stage whole planes (several
// chunks each), and it lives two to three times as long as a tile of the interior.  With the ranges
// in storage order the top tip came LAST: a few dozen such wavefronts running on after every other
// had finished, 35 us at the end of a 290 us launch (the last slab of the 8-slab rehearsal, whose
// list ends with the tip: GRBM_GUI_ACTIVE + 10 % for the same SQ_WAVE_CYCLES as the first slab's,
// profiles/r04_slab_pmc_by_rank.json).  Now both tips are started within the first half of a
// launch, and it ends in the middle of the list, among tiles that are all alike.
#ifndef YA_XCD_RANGES
#define YA_XCD_RANGES 2  /* contiguous ranges of tiles per XCD (1 = plain eighths) */
#endif
#ifndef YA_XCD_OUTSIDE_IN
#define YA_XCD_OUTSIDE_IN 1  /* 0 = ranges in storage order (A/B) */
#endif
template<int RANGES = YA_XCD_RANGES>
__device__ __forceinline__ int xcd_contiguous_tile(const int block, const int n_blocks)
{
    // slots of a multiple of 8 blocks each (block and block - k * part then sit on the same XCD);
    // the last slot in time takes the remainder
    const int part = (n_blocks / RANGES) & ~7;
    if (RANGES == 1 || part == 0) return xcd_eighth_tile(block, n_blocks);
    const int p = min(block / part, RANGES - 1);
    const int first_block = p * part;
    const int len = p == RANGES - 1 ? n_blocks - first_block : part;
#if YA_XCD_OUTSIDE_IN
    // slot p works on range r of the list: 0, R - 1, 1, R - 2, ...; the last slot on range R / 2, which
    // is therefore the one that holds the remainder
    constexpr int LONG_RANGE = RANGES / 2;
    const bool from_back = p & 1;
    const int r = from_back ? RANGES - 1 - (p - 1) / 2 : p / 2;
    const int start = r * part + (r > LONG_RANGE ? n_blocks - RANGES * part : 0);
    return start + xcd_eighth_tile(block - first_block, len, from_back);
#else
    return first_block + xcd_eighth_tile(block - first_block, len);
#endif
}

// Test hook: the same for ya::reciprocal (dtypes.cuh) against 1.0f / x.
__global__ void check_reciprocal_all(
    unsigned first, unsigned last, unsigned long long* mismatches)
{
    unsigned long long bad = 0;
    for (unsigned long long u = (unsigned long long)first + blockIdx.x * blockDim.x + threadIdx.x;
         u <= last; u += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __int_as_float((int)(unsigned)u);
        const float a = reciprocal(x), b = 1.0f / x;
        if (__float_as_int(a) != __float_as_int(b) && !(a != a && b != b)) bad++;
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Optional HIP-event timing of the force-kernel launches (bench.py's roofline
// leg).  The pair of events handed out by next() is attached to the kernel's own
// dispatch (hipExtLaunchKernelGGL), so that timing a launch puts no extra packet
// into the stream.  Even so a timed launch is a few microseconds slower end to end,
// so only every `stride`-th launch is timed (use an odd stride to see both Heun
// stages).  Disabled by default: next() then hands out null events.
class Profiler {
public:
    void enable(bool on, int every = 1)
    {
        enabled = on;
        stride = every > 0 ? every : 1;
        seen = 0;
    }
    bool active() const { return enabled; }
    void next(hipEvent_t* start, hipEvent_t* stop)
    {
        *start = *stop = nullptr;
        if (!enabled || seen++ % stride != 0) return;
        while (used + 2 > events.size()) {
            hipEvent_t e;
            YA_CHECK((int)hipEventCreate(&e));
            events.push_back(e);
        }
        *start = events[used++];
        *stop = events[used++];
    }
    // Sum of (after - before) over the recorded launches; resets the record.
    void read(double* total_ms, int* launches)
    {
        YA_CHECK((int)hipDeviceSynchronize());
        double ms = 0;
        for (size_t k = 0; k + 1 < used; k += 2) {
            float span = 0;
            YA_CHECK((int)hipEventElapsedTime(&span, events[k], events[k + 1]));
            ms += span;
        }
        if (total_ms) *total_ms = ms;
        if (launches) *launches = (int)(used / 2);
        used = 0;
    }
    ~Profiler()
    {
        for (auto e : events) (void)hipEventDestroy(e);
    }

private:
    bool enabled = false;
    int stride = 1;
    long seen = 0;
    size_t used = 0;
    std::vector<hipEvent_t> events;
};

template<typename Pt>
bool is_no_gen_forces(const Generic_forces<Pt>& f)
{
    using Fn = void (*)(const int, const Pt* __restrict__, Pt*);
    auto* target = f.template target<Fn>();
    return target && *target == static_cast<Fn>(&no_gen_forces<Pt>);
}

// dX = gen + F, then the friction term of add_rhs (solvers.cuh:146-161).
template<typename Pt>
__device__ __forceinline__ Pt store_rhs(
    Pt* __restrict__ d_dX, int i, bool has_gen, Pt F, float3 sum_v, float sum_friction)
{
    Pt dX;
    if (has_gen) {
        dX = d_dX[i];
        dX += F;
    } else {
        dX = F;
    }
    if (sum_friction > 0) {
        dX.x += sum_v.x / sum_friction;
        dX.y += sum_v.y / sum_friction;
        dX.z += sum_v.z / sum_friction;
    }
    d_dX[i] = dX;
    return dX;
}

// One pair (i, j) of the all-pairs force: the functors' terms added to cell i's running sums, in the statements
// and the order every one-lane all-pairs loop has (tile_force_rows below, ya::ens::whole_steps in
// include/ensemble.cuh).  vj is read only where the friction is not zero.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__device__ __forceinline__ void tile_pair(const Pt Xi, const Pt& Xj, const float3& vj, const int i, const int j, Pt& F,
    float3& sum_v, float& sum_friction)
{
    Pt r = Xi - Xj;
    float dist = dist3(r.x, r.y, r.z);
    F += pw_int(Xi, r, dist, i, j);
    float friction = pw_friction(Xi, r, dist, i, j);
    sum_friction += friction;
    if (friction != 0) {
        float3 v = vj;
        sum_v.x += friction * v.x;
        sum_v.y += friction * v.y;
        sum_v.z += friction * v.z;
    }
}

// All-pairs force (replaces compute_tile, solvers.cuh:284-322): j ascending,
// functor called for every (i, j) including i == j.
// The body, for one system's n rows at d_X / d_old_v / d_dX: the workgroup is the system's `block`-th and
// serves TILE_BLOCK of its rows; the functors are handed the ids id_base + row (an ensemble's replica starts
// at id_base, include/ensemble.cuh; a lone system's constant 0 folds away).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__device__ __forceinline__ void tile_force_rows(const int n, const int block, const int id_base,
    const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v, Pt* __restrict__ d_dX, const bool has_gen)
{
    __shared__ Pt sh_X[TILE_POINTS];
    __shared__ float3 sh_v[TILE_POINTS];

    const int local = block * TILE_BLOCK + threadIdx.x;
    const int i = id_base + local;
    Pt Xi = ya::zero<Pt>();
    if (local < n) Xi = d_X[local];
    Pt F = ya::zero<Pt>();
    float3 sum_v{0.f, 0.f, 0.f};
    float sum_friction = 0;
    for (int tile_start = 0; tile_start < n; tile_start += TILE_POINTS) {
        const int n_tile = min(TILE_POINTS, n - tile_start);
        __syncthreads();
        for (int k = threadIdx.x; k < n_tile; k += TILE_BLOCK) {
            sh_X[k] = d_X[tile_start + k];
            sh_v[k] = d_old_v[tile_start + k];
        }
        __syncthreads();
        if (local < n) {
            // unrolled: the pairs' distance / functor chains are independent and overlap,
            // the sums stay in j order
#ifndef YA_TILE_UNROLL
#define YA_TILE_UNROLL 4
#endif
#pragma unroll YA_TILE_UNROLL
            for (int k = 0; k < n_tile; k++) {
                const int j = id_base + tile_start + k;
                tile_pair<Pt, pw_int, pw_friction>(Xi, sh_X[k], sh_v[k], i, j, F, sum_v, sum_friction);
            }
        }
    }
    if (local < n) store_rhs(d_dX, local, has_gen, F, sum_v, sum_friction);
}
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(TILE_BLOCK) void tile_force(const int n,
    const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v, Pt* __restrict__ d_dX,
    const bool has_gen)
{
    tile_force_rows<Pt, pw_int, pw_friction>(n, blockIdx.x, 0, d_X, d_old_v, d_dX, has_gen);
}

// The two phases of the several-lanes all-pairs kernels (tile_force_coop_rows below, ya::ens::whole_stage_force_coop
// in include/ensemble.cuh), written once: what a pair leaves in LDS, and the order its terms are added in.
// (a) One pair (i, j), the partner being row k of X and of old_v (LDS): its terms {F (NF), friction,
// friction * old_v (3)} are handed to store(c, term), c = 0 .. NF + 3, which leaves term c in column j of the
// caller's [component][j] rows.  (Arrays and a row, not references to the partner: old_v's row is then addressed
// where it is read, after the functors, and no address lives across their calls.)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Store>
__device__ __forceinline__ void coop_pair_terms(const Pt Xi, const Pt* X, const float3* old_v, const int k, const int i,
    const int j, const Store& store)
{
    constexpr int NF = N_floats<Pt>::value;
    Pt r = Xi - X[k];
    float dist = dist3(r.x, r.y, r.z);
    const Pt f = pw_int(Xi, r, dist, i, j);
    const float friction = pw_friction(Xi, r, dist, i, j);
#pragma unroll
    for (int c = 0; c < NF; c++) store(c, field(f, c));
    store(NF, friction);
    // the old_v term only where the friction is not zero (solvers.cuh:312-316): a +0
    // term instead changes no bit of a sum that started at +0 (such a sum never is -0)
    const float3 v = old_v[k];
    store(NF + 1, friction != 0 ? friction * v.x : 0.f);
    store(NF + 2, friction != 0 ? friction * v.y : 0.f);
    store(NF + 3, friction != 0 ? friction * v.z : 0.f);
}
// (b) sum + terms[0] + terms[1] + ... + terms[n_terms - 1], added one after the other in that order.  `terms` is
// 16-byte aligned.  Sixteen terms per trip: four 16-byte LDS reads in flight, then the adds in order.
__device__ __forceinline__ float coop_ordered_sum(float sum, const float* terms, const int n_terms)
{
    const float4* terms4 = reinterpret_cast<const float4*>(terms);
    int jj = 0;
    for (; jj + 16 <= n_terms; jj += 16) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; u++) p[u] = terms4[jj / 4 + u];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            sum += p[u].x;
            sum += p[u].y;
            sum += p[u].z;
            sum += p[u].w;
        }
    }
    for (; jj < n_terms; jj++) sum += terms[jj];
    return sum;
}

// The same all-pairs force with 16 or 64 lanes per cell (opt-in: Tile_computer::lanes_per_cell).
// All pairs of 800 cells are only 13 wavefronts for tile_force, each lane walking its 800
// partners alone: 0.19 ms per launch on a 256-CU chip.  Here a 256-thread workgroup owns 16 or 4
// cells; for every tile of up to 512 partners each cell's lanes evaluate eight pairs apiece and
// leave {F, friction, friction * old_v} in LDS, then ONE lane per component runs that
// component's sum over the tile in ascending j -- every per-cell sum is still accumulated in
// exactly the reference's order, and results are bit-identical to tile_force.  What changes:
// the functor is called for one i from several lanes at once, so functors that update per-cell
// state non-atomically (d_mes_nbs[i] += 1, examples/passive_growth.cu:48-51) must keep the
// default of one lane per cell.
// Partners per tile of that kernel: a multiple of 64, at most 512, whose terms -- N_floats + 4 components for each of the
// workgroup's 256 / COOP_LANES cells -- fill at most 56 KiB of LDS.  Less than 64 (16 lanes per cell from 11 floats on)
// means that the kernel does not exist for the type: Tile_computer asks before it names it.
template<typename Pt, int COOP_LANES>
constexpr int tile_coop_partners()
{
    constexpr int fit = (57344 / ((256 / COOP_LANES) * (N_floats<Pt>::value + 4) * 4)) / 64 * 64;
    return fit > 512 ? 512 : fit;
}
// The body, with tile_force_rows' arguments: the workgroup serves 256 / COOP_LANES of the system's rows.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int COOP_LANES>
__device__ __forceinline__ void tile_force_coop_rows(const int n, const int block, const int id_base,
    const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v, Pt* __restrict__ d_dX, const bool has_gen)
{
    constexpr int COOP_CELLS = 256 / COOP_LANES;
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;  // components summed per cell: F (NF), friction, friction * old_v (3)
    // partners per tile: a multiple of 64 whose terms fill at most 56 KiB of LDS
    constexpr int TILE = tile_coop_partners<Pt, COOP_LANES>();
    static_assert(TILE >= 64, "point type too large for tile_force_coop");
    constexpr int THREADS = COOP_CELLS * COOP_LANES;
    constexpr int LOADS = (TILE + THREADS - 1) / THREADS;  // partners a thread carries per tile
    constexpr int SLOTS = (NC + COOP_LANES - 1) / COOP_LANES;
    __shared__ __attribute__((aligned(16))) float sh_part[COOP_CELLS][NC][TILE];  // one tile's terms, [cell][component][j]
    __shared__ Pt sh_X[TILE];                        // the tile's partners
    __shared__ float3 sh_v[TILE];
    __shared__ float sh_sum[COOP_CELLS][NC];

    const int cell = threadIdx.x / COOP_LANES, lane = threadIdx.x % COOP_LANES;
    const int local = block * COOP_CELLS + cell;
    const int i = id_base + local;
    const bool active = local < n;
    Pt Xi = ya::zero<Pt>();
    if (active) Xi = d_X[local];
    float acc[SLOTS];  // this lane's component sums (components lane, lane + COOP_LANES, ...)
#pragma unroll
    for (int a = 0; a < SLOTS; a++) acc[a] = 0.f;

    // the next tile's partners travel from global memory while the current tile is worked on
    Pt x_next[LOADS];
    float3 v_next[LOADS];
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const int j = threadIdx.x + k * THREADS;
        x_next[k] = ya::zero<Pt>();
        v_next[k] = float3{0.f, 0.f, 0.f};
        if (j < TILE && j < n) {
            x_next[k] = d_X[j];
            v_next[k] = d_old_v[j];
        }
    }
    for (int tile_start = 0; tile_start < n; tile_start += TILE) {
        const int n_tile = min(TILE, n - tile_start);
#pragma unroll
        for (int k = 0; k < LOADS; k++) {
            const int t = threadIdx.x + k * THREADS;
            if (t < TILE) {
                sh_X[t] = x_next[k];
                sh_v[t] = v_next[k];
                const int j_next = tile_start + TILE + t;
                if (j_next < n) {
                    x_next[k] = d_X[j_next];
                    v_next[k] = d_old_v[j_next];
                }
            }
        }
        __syncthreads();
        // (a) the tile's pair terms: lane l takes partners l, l + COOP_LANES, ...
        if (active) {
#pragma unroll 4
            for (int jj = lane; jj < n_tile; jj += COOP_LANES) {
                const int j = id_base + tile_start + jj;
                coop_pair_terms<Pt, pw_int, pw_friction>(
                    Xi, sh_X, sh_v, jj, i, j, [&](const int c, const float term) { sh_part[cell][c][jj] = term; });
            }
        }
        __syncthreads();
        // (b) one lane per component adds the tile's terms in ascending j
#pragma unroll
        for (int a = 0; a < SLOTS; a++) {
            const int c = lane + COOP_LANES * a;
            if (c < NC && active) acc[a] = coop_ordered_sum(acc[a], &sh_part[cell][c][0], n_tile);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < SLOTS; a++) {
        const int c = lane + COOP_LANES * a;
        if (c < NC) sh_sum[cell][c] = acc[a];
    }
    __syncthreads();
    if (active && lane == 0) {
        Pt F;
#pragma unroll
        for (int c = 0; c < NF; c++) field(F, c) = sh_sum[cell][c];
        store_rhs(d_dX, local, has_gen, F,
            float3{sh_sum[cell][NF + 1], sh_sum[cell][NF + 2], sh_sum[cell][NF + 3]}, sh_sum[cell][NF]);
    }
}
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int COOP_LANES>
__global__ __launch_bounds__(256) void tile_force_coop(const int n,
    const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v, Pt* __restrict__ d_dX,
    const bool has_gen)
{
    tile_force_coop_rows<Pt, pw_int, pw_friction, COOP_LANES>(n, blockIdx.x, 0, d_X, d_old_v, d_dX, has_gen);
}

// Row r of the 27-cube stencil in the reference's d_nhood order
// (solvers.cuh:472-483): rows of three consecutive cube ids centred on
// 0, -gs, +gs, then the same three shifted by -gs^2, then by +gs^2.
__device__ __forceinline__ int stencil_row_offset(int row, int gs)
{
    const int dy = row % 3, dz = row / 3;
    const int oy = dy == 0 ? 0 : (dy == 1 ? -gs : gs);
    const int oz = dz == 0 ? 0 : (dz == 1 ? -gs * gs : gs * gs);
    return oy + oz;
}

// Grid force (replaces compute_cube, solvers.cuh:430-463).  Thread s owns
// sorted slot s.  offs[c] = first slot of cube c, so the cubes c-1, c, c+1 of a
// stencil row are the contiguous slots [offs[c-1], offs[c+2]).

// The first 16 bytes of a staged cell (x, y, z and one more word).  Entries whose
// size is a multiple of 16 bytes are read as one 16-byte LDS access: 4 LDS cycles
// per wavefront, where the 12-byte form the compiler picks for x, y, z alone takes
// 8 (MI355X_MICROARCH.md, section LDS).  keep_wide() is what stops it narrowing.
template<typename Pt>
__device__ __forceinline__ float4 staged_words(const Entry<Pt>* e)
{
    if constexpr (sizeof(Entry<Pt>) % 16 == 0)
        return *reinterpret_cast<const float4*>(e);
    else
        return float4{e->X.x, e->X.y, e->X.z, 0.f};
}
__device__ __forceinline__ void keep_wide(const float4& w) { asm volatile("" ::"v"(w.w)); }

template<typename Pt>
__device__ __forceinline__ float dist2_to(const Pt& a, const float4 b)
{
    const float dx = a.x - b.x;
    const float dy = a.y - b.y;
    const float dz = a.z - b.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

template<typename Pt>
__device__ __forceinline__ float dist2(const Pt& a, const Pt& b)
{
    const float dx = a.x - b.x;
    const float dy = a.y - b.y;
    const float dz = a.z - b.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// Smallest binary32 t with sqrtf(t) >= cube_size.  sqrtf is monotonic and
// correctly rounded on host and device, so `d2 < t` is exactly the reference's
// `dist < cube_size` (solvers.cuh:450) without a square root per candidate.
inline float cutoff_squared(float cube_size)
{
    float t = cube_size * cube_size;
    while (t > 0 && sqrtf(t) >= cube_size) t = nextafterf(t, 0.f);
    while (sqrtf(t) < cube_size) t = nextafterf(t, INFINITY);
    return t;
}

// A model's pairwise functor is inlined where the grid kernels call it, whatever its size.  Left to
// the inliner, a functor with libm calls in it (bending_force's sinf / cosf) stays a function that is
// called per pair: it then re-reads the device symbols it uses (`d_type`, `d_mes_nbs` ...) and cell i's
// own entries for every pair, each of them a round trip in front of the arithmetic.
#ifndef YA_CALL_INLINED
#define YA_CALL_INLINED [[clang::always_inline]]
#endif

// Row bounds of a plane of the stencil for a workgroup that owns the cubes [c_lo, c_hi] and a lane in
// cube c: six workgroup-uniform and six per-lane reads of offs[].  Those of plane p + 1 are requested
// while plane p computes, so that a plane's staging loads do not queue behind a round trip to L2 for
// its bounds.  Expects next_lo / next_hi / next_begin / next_end [3], c_lo, c_hi, c, gs, n_cubes, offs.
#define YA_ROW_BOUNDS(plane_)                                                          \
    _Pragma("unroll") for (int r = 0; r < 3; r++)                                      \
    {                                                                                  \
        const int off = stencil_row_offset(3 * (plane_) + r, gs);                      \
        /* The reference indexes cube_start/end without bounds checks               */ \
        /* (solvers.cuh:444); out-of-grid cubes are treated as empty here.          */ \
        next_lo[r] = offs[min(max(c_lo + off - 1, 0), n_cubes)];                       \
        next_hi[r] = offs[min(max(c_hi + off + 2, 0), n_cubes)];                       \
        next_begin[r] = offs[min(max(c + off - 1, 0), n_cubes)];                       \
        next_end[r] = offs[min(max(c + off + 2, 0), n_cubes)];                         \
    }

}  // namespace ya
#ifdef YA_EXPERIMENTAL_FORCE_VARIANTS
#include "force_variants.cuh"  // tools/ab/: grid_force_direct, grid_force (byte FIFO) -- A/B baselines for tests and tools (-Itools/ab)
#endif
namespace ya {

// ---------------------------------------------------------------------------------
// grid_force_bits (the default): the same two-phase kernel with the hit list kept as a BIT
// STREAM (one bit per tested candidate, in the reference's order) instead of a byte FIFO,
// in one-wavefront workgroups.
//
//   phase 1  per candidate: one 16-byte LDS read, the squared distance and
//            `m = 2 m + (d2 < cut2)` -- a compare and an add-with-carry.  A word is
//            stored to LDS once per four candidates (one ds_write_b32 where the byte
//            FIFO issued four ds_write_b8) in [word][thread] order: no bank conflicts.
//            Rows are padded to a multiple of four bits, so there is no one-candidate
//            tail loop: the last group of a row is tested under a mask.
//   phase 2  pops the set bits highest first (= ascending candidate order), two per trip:
//            the second hit's LDS / global loads are in flight while the first one's
//            arithmetic runs (the sums stay in order).  The bit position gives the
//            staged cell through three per-lane row offsets; the next word of the stream
//            is requested one trip ahead.
//
// A pass covers 32 * YA_MASK_WORDS candidate bits per lane.  A plane's three rows fit
// into one pass at any density a model normally runs at (~90 candidates per plane at
// rho = 9.8); a wavefront in which some lane has more falls back to one pass per row
// stretch.  A workgroup is ONE wavefront (64 cells): nothing waits at a workgroup barrier
// for a slower wavefront, launches of 10^4..10^5 cells spread over four times as many
// CUs, and the workgroup needs 7 KiB of LDS.  MI355X, same box (tools/micro/force_ab.hip):
// 242 us per 1 M-cell launch against 260 us for round 1's byte-FIFO kernel, 62 against 75 us at 10^5 cells,
// 803 against 853 us at 4 M.  What bounds it is the VALU issue rate.
// Results are bit-identical to the earlier kernels' (tools/ab/force_variants.cuh): same candidates, same
// order, same arithmetic.
// The friction terms of one pair (solvers.cuh:309-313, :453-458): sum_friction += friction,
// sum_v += friction * old_v[j].  For the default functor friction_w_neighbour the coefficient f
// is 0 or 1, so f * v is exact and `fmaf(f, v, sum)` is `sum + f * v` with its one rounding: the
// reference's bits, unconditionally as the reference adds it (a non-finite old_v poisons the sum
// there and here), in one instruction per component where `sum += nb ? v : 0` took two (round 6:
// 242 -> 237 us per 1 M-cell launch, profiles/r06_force_ab.jsonl; round 3's selections had been
// -2.6 % against the multiply-and-add before them).
template<typename Pt, Pairwise_friction<Pt> pw_friction>
__device__ __forceinline__ void pair_friction(const Pt& Xi, const Pt& r, const float dist, const int i,
    const int j, const float4& v, float3& sum_v, float& sum_friction)
{
    if constexpr (pw_friction == &friction_w_neighbour<Pt>) {
        const bool nb = (i != j) & (dist < 1.f);
        const float f = nb ? 1.f : 0.f;
        sum_friction += f;
        sum_v.x = fmaf(f, v.x, sum_v.x);
        sum_v.y = fmaf(f, v.y, sum_v.y);
        sum_v.z = fmaf(f, v.z, sum_v.z);
    } else {
        const float friction = pw_friction(Xi, r, dist, i, j);
        sum_friction += friction;
        if (friction != 0) {
            sum_v.x += friction * v.x;
            sum_v.y += friction * v.y;
            sum_v.z += friction * v.z;
        }
    }
}

// Hooks of tools/micro/force_trace.hip (when and where every workgroup of a launch ran): empty
// unless tools/ab/force_trace.cuh was included first.
#ifndef YA_BITS_PROBE_BEGIN
#define YA_BITS_PROBE_BEGIN
#define YA_BITS_PROBE_END(tile_)
#endif
namespace bits {
#ifndef YA_BITS_BLOCK
#define YA_BITS_BLOCK 64
#endif
#ifndef YA_MASK_WORDS
#define YA_MASK_WORDS 4
#endif
#ifndef YA_BITS_POPS
#define YA_BITS_POPS 2  /* hits popped per trip of phase 2 (1 or 2), three-float points */
#endif
#ifndef YA_BITS_POPS_WIDE
#define YA_BITS_POPS_WIDE 2  /* the same for wider points (A/B knob: one pop per trip saves 10 VGPRs of config */
#endif                       /* 4's 146 and is 3 % slower there: two hits' memory accesses in flight matter more) */
// Wavefronts per SIMD the register allocator must leave room for (A/B knob).  Default 1 = the
// compiler's own choice.  Measured on config 4 (1.16 M Po_cell, relu_w_epithelium: 146 VGPRs, three
// wavefronts per SIMD, 78 % of wave cycles at s_waitcnt): forcing four (128 VGPRs + 8 spilled)
// made the launch SLOWER, 1431 -> 1615 us -- that kernel is bound by the address path of the
// functor's own global accesses (d_type[i], d_type[j], d_mes_nbs[i] += 1 by original id: 64 cache
// lines per wavefront instruction, TA 73 % busy), and more wavefronts only queue there.
// Round 4: once the MODEL keeps its ids in cube order (Solution::renumber) those accesses are
// neighbouring lines, and while the functor was still a called function four wavefronts per SIMD and
// one hit per trip were the faster build there, 652 -> 585 us per launch (profiles/r04_cfg4_renumber_ab.txt:
// a second build of the kernel for renumbered models).  With the functor inlined (YA_CALL_INLINED) the
// compiler's own choice and two hits per trip are the fastest again, renumbered or not: 559-566 us
// (profiles/r04_inline_ab.txt) -- a four-wavefront build then spills the force sums inside the loop
// (752 us; 1000 us with `int* d_type`) -- and the second build is gone.
#ifndef YA_BITS_MIN_WAVES_WIDE
#define YA_BITS_MIN_WAVES_WIDE 1
#endif
template<typename Pt>
struct Min_waves {
    static constexpr int value = sizeof(Pt) <= 16 ? 1 : YA_BITS_MIN_WAVES_WIDE;
};
template<typename Pt>
struct Pops {
    static constexpr int value = sizeof(Pt) <= 16 ? YA_BITS_POPS : YA_BITS_POPS_WIDE;
};
constexpr int BLOCK = YA_BITS_BLOCK;
constexpr int WORDS = YA_MASK_WORDS;
constexpr int PASS_BITS = 32 * WORDS;
static_assert(BLOCK % 32 == 0, "phase 2 steps its word pointer by BLOCK / 32 elements per bit position");
using Lds_word = __attribute__((address_space(3))) unsigned;

template<typename Pt>
struct Stage {
#ifndef YA_BITS_STAGE_CELLS
#define YA_BITS_STAGE_CELLS (3 * YA_BITS_BLOCK + 160)
#endif
    // 16- and 24-byte entries: 352 cells (7 / 9.7 KiB per wavefront with the masks: 5 / 4 wavefronts
    // per SIMD); 32-byte entries (7-float points): 256 cells = 9.5 KiB, so that a fourth wavefront
    // fits the CU's LDS (352 were 12.6 KiB: three) -- denser planes are staged in chunks
    static constexpr int value = sizeof(Entry<Pt>) <= 24 ? YA_BITS_STAGE_CELLS
                                 : (sizeof(Entry<Pt>) <= 32 ? 256 : YA_BITS_STAGE_CELLS / 2);
};

// m = 2 m + (d2 < cut2)
__device__ __forceinline__ void shift_in(unsigned& m, const float d2, const float cut2)
{
    asm("v_cmp_gt_f32 vcc, %2, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
        : "+v"(m)
        : "v"(d2), "s"(cut2)
        : "vcc");
}

// Phase 2 gathers old_v as `sorted_v` + a 32-bit unsigned BYTE offset (one uniform base, no 64-bit address
// built per hit) while every slot's offset fits: 16 n < 2^32.  Grid_computer::forces asks here where it picks
// the launch; larger systems keep the 64-bit form (OFF32 = false).
__host__ __device__ constexpr bool offsets_fit_32_bits(const long long n)
{
    return n >= 0 && 16ll * n < (1ll << 32);
}

// What a pass may know about its hits before it pops the first one (Grid_computer::pass_facts).  A pass that knows
// drains its stream through a phase 2 compiled under that knowledge; what the pass computes does not change.
//   DISTINCT  no hit is the lane's own cell (i != j).  A cell is its own candidate in one stencil row of its own plane:
//             ids are unique per slot, so the fact holds iff no active lane's own slot lies in one of the pass'
//             three candidate ranges -- which the caller tests on the ranges themselves, wave-uniformly, not on the
//             plane number (in a grid of one cube an axis the rows of the planes below and above are the cell's own
//             cube too).  spring's `i == j ? 0 : dF` and friction_w_neighbour's `i != j` then fold away.
//   NEAR      every hit has dist < 1.  A hit is a candidate with d2 < cut2, dist2_to (phase 1) and the statements
//             in front of dist3 (phase 2) are the same subtractions, product and two fmaf, and exact_sqrt is sqrtf
//             for every bit pattern: where cut2 <= cutoff_squared(1) -- the smallest binary32 whose root reaches 1
//             -- sqrtf(d2) < 1.  Decided once per launch on the host (launch_facts).
// Under both, friction_w_neighbour's coefficient is the constant 1: sum_friction += 1 and three plain adds
// (fmaf(1, v, s) and s + v round alike; a non-finite old_v poisons the sum either way).
// The fast tier keeps the generic body alone: NEAR is not true there (its bare v_sqrt_f32, <= 1 ulp, can return 1 just
// below the cut-off), and DISTINCT alone measured 2 us per step SLOWER than the generic body alone at 10^6 cells
// (DESIGN.md section 6, round 10).
#ifdef YA_ARITH_FAST
constexpr bool FACT_BODIES = false;
#else
constexpr bool FACT_BODIES = true;
#endif
constexpr int FACT_DISTINCT = 1, FACT_NEAR = 2;
// The facts a launch with cut-off cut2 may use.  `setting` is Grid_computer::pass_facts: 0 none (generic bodies only),
// 1 (default) both, 2 / 3 DISTINCT / NEAR alone (A/B).  Any setting gives the same bits.
inline int launch_facts(const int setting, const float cut2)
{
    if (!FACT_BODIES) return 0;
    int facts = setting == 0 ? 0 : (setting == 2 ? FACT_DISTINCT : (setting == 3 ? FACT_NEAR : FACT_DISTINCT | FACT_NEAR));
    if (!(cut2 <= cutoff_squared(1.0f))) facts &= ~FACT_NEAR;
    return facts;
}

// Phase 1 of a pass leaves the bit stream in LDS and these in registers: bits emitted, where segments 1 and 2 begin
// in the stream, and per segment LDS index - bit position.
struct Scan {
    int p, p1, p2, d0, d1, d2;
};

// One pass: up to three candidate segments [b_r, e_r) of the staged cells (LDS indices;
// empty if b_r >= e_r), at most PASS_BITS bits after padding each to a multiple of four.
// shift_r turns an LDS index of segment r into a slot of the sorted arrays.
// scan() is phase 1, drain() phase 2 (DISTINCT, NEAR: above), pass() one after the other.
template<typename Pt>
__device__ __forceinline__ Scan scan(const Entry<Pt>* __restrict__ sh_e, Lds_word* const words,
    const int b0, const int e0, const int b1, const int e1, const int b2, const int e2, const Pt& Xi, const float cut2)
{
    // ---- phase 1 ----
    unsigned m = 0;
    int p = 0;  // bits emitted
    Lds_word* mp = words;
#define YA_BITS_GROUP(end_, masked_)                                                   \
    {                                                                                  \
        float4 w[4];                                                                   \
        float d2[4];                                                                   \
        _Pragma("unroll") for (int u = 0; u < 4; u++) w[u] = staged_words(&sh_e[t + u]); \
        _Pragma("unroll") for (int u = 0; u < 4; u++)                                  \
        {                                                                              \
            d2[u] = dist2_to(Xi, w[u]);                                                \
            keep_wide(w[u]);                                                           \
            if (masked_) d2[u] = t + u < (end_) ? d2[u] : INFINITY;                    \
        }                                                                              \
        _Pragma("unroll") for (int u = 0; u < 4; u++) shift_in(m, d2[u], cut2);        \
        p += 4;                                                                        \
        *mp = m; /* the word's last store, when it is full, is the one that counts */  \
        const bool full = (p & 31) == 0;                                               \
        mp += full ? BLOCK : 0;                                                        \
        m = full ? 0u : m;                                                             \
    }
#define YA_BITS_SEGMENT(begin_, end_)                                                  \
    {                                                                                  \
        int t = (begin_);                                                              \
        for (; t + 4 <= (end_); t += 4) YA_BITS_GROUP(end_, false)                     \
        if (t < (end_)) YA_BITS_GROUP(end_, true)                                      \
    }
    const int d0 = b0;  // LDS index = bit position + d_r inside segment r
    YA_BITS_SEGMENT(b0, e0)
    const int p1 = p, d1 = b1 - p1;
    YA_BITS_SEGMENT(b1, e1)
    const int p2 = p, d2_ = b2 - p2;
    YA_BITS_SEGMENT(b2, e2)
#undef YA_BITS_SEGMENT
#undef YA_BITS_GROUP
    if (p & 31) *mp = m << (32 - (p & 31));  // left-align the last, partial word
    return {p, p1, p2, d0, d1, d2_};
}

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V, bool GLOBAL_IDS,
    bool OFF32, bool DISTINCT, bool NEAR>
__device__ __forceinline__ void drain(const Entry<Pt>* __restrict__ sh_e, const float4* __restrict__ sh_v,
    Lds_word* const words, const Scan& sc, const int shift0, const int shift1, const int shift2,
    const float4* __restrict__ sorted_v, const Pt& Xi, const int i, Pt& F, float3& sum_v, float& sum_friction,
    const int* __restrict__ global_id, const int id_base)
{
    static_assert(!(DISTINCT && GLOBAL_IDS), "a slab's launches keep the generic body");
    constexpr int POPS = Pops<Pt>::value;
    const int p = sc.p, p1 = sc.p1, p2 = sc.p2, d0 = sc.d0, d1 = sc.d1, d2_ = sc.d2;
    // ---- phase 2 ----
    // A hit at bit position q of segment r is staged cell q + d_r, sorted slot q + d_r + shift_r.  The three
    // per-lane BYTE offsets of either are formed once per pass; a hit then costs two compares, the selects and
    // one shift-and-add per address (round 7: the slot had been an index sum, a select of the uniform shifts
    // -- moved from SGPRs to VGPRs every trip -- and a 64-bit shift-and-add per hit).
    constexpr unsigned ENTRY = sizeof(Entry<Pt>);
    constexpr bool ONE_OFFSET = ENTRY == sizeof(float4);  // sh_e and sh_v share the byte offset
    const unsigned lds0 = ENTRY * (unsigned)d0, lds1 = ENTRY * (unsigned)d1, lds2 = ENTRY * (unsigned)d2_;
    const unsigned gat0 = 16u * (unsigned)(d0 + shift0), gat1 = 16u * (unsigned)(d1 + shift1),
                   gat2 = 16u * (unsigned)(d2_ + shift2);
    Lds_word* const rp_end = words + ((p + 31) >> 5) * BLOCK;  // past this lane's last word
    unsigned cur = p > 0 ? words[0] : 0u;
    Lds_word* rp = words + BLOCK;  // the word after the current one
    unsigned nxt = *rp;  // one spare row keeps this in bounds
    int wbase = 0;
#define YA_BITS_LOAD(q_, other_, v_)                                                   \
    {                                                                                  \
        const bool in2 = (q_) >= p2, in1 = (q_) >= p1;                                 \
        if constexpr (OFF32 && ONE_OFFSET) {                                           \
            const unsigned at = ENTRY * (unsigned)(q_) + (in2 ? lds2 : (in1 ? lds1 : lds0)); \
            other_ = *(const Entry<Pt>*)((const char*)sh_e + at);                      \
            if (STAGE_V) v_ = *(const float4*)((const char*)sh_v + at);                \
        } else {                                                                       \
            const int t = (q_) + (in2 ? d2_ : (in1 ? d1 : d0));                        \
            other_ = sh_e[t];                                                          \
            if (STAGE_V) v_ = sh_v[t];                                                 \
            if (!STAGE_V && !OFF32) v_ = sorted_v[(unsigned)(t + (in2 ? shift2 : (in1 ? shift1 : shift0)))]; \
        }                                                                              \
        if constexpr (OFF32 && !STAGE_V) {                                             \
            const unsigned at = 16u * (unsigned)(q_) + (in2 ? gat2 : (in1 ? gat1 : gat0)); \
            v_ = *(const float4*)((const char*)sorted_v + (size_t)at);                 \
        }                                                                              \
    }
#define YA_BITS_PAIR(other_, v_)                                                       \
    {                                                                                  \
        Pt r = Xi - other_.X;                                                          \
        float dist = dist3(r.x, r.y, r.z);                                             \
        const int j = (GLOBAL_IDS ? global_id[other_.id] : other_.id) + id_base;       \
        /* what the pass knows, said on this side of the functors (as YA_CALL_INLINED is) */ \
        if constexpr (DISTINCT) __builtin_assume(i != j);                              \
        if constexpr (NEAR) __builtin_assume(dist < 1.f);                              \
        YA_CALL_INLINED F += pw_int(Xi, r, dist, i, j);                                \
        pair_friction<Pt, pw_friction>(Xi, r, dist, i, j, v_, sum_v, sum_friction);    \
    }
#ifdef YA_BITS_MEASUREMENT_PROBES  // measurement builds only (tools/micro/force_ab.hip; -Itools/ab): the balance and phase-1 probes
#include "bits_probe.inc"
#endif
    while (cur != 0 || rp < rp_end) {
        const int step = cur == 0 ? 32 : 0;  // refill (then rp < rp_end): one select moves both wbase and rp
        cur = cur == 0 ? nxt : cur;
        wbase += step;
        rp += step * (BLOCK / 32);
        nxt = *rp;
        if (cur != 0) {
            // up to POPS hits of the word: the loads of the later ones are issued before
            // the first one's arithmetic (a hit that is not there repeats the one before it)
            int pos[POPS];
            bool have[POPS];
            Entry<Pt> other[POPS];
            float4 v[POPS];
#pragma unroll
            for (int u = 0; u < POPS; u++) {
                have[u] = cur != 0;
                pos[u] = have[u] ? __builtin_clz(cur) : pos[u > 0 ? u - 1 : 0];
                cur = have[u] ? cur & (0x7fffffffu >> pos[u]) : cur;
                YA_BITS_LOAD(wbase + pos[u], other[u], v[u])
            }
            YA_BITS_PAIR(other[0], v[0])
#pragma unroll
            for (int u = 1; u < POPS; u++)
                if (have[u]) YA_BITS_PAIR(other[u], v[u])
        }
    }
#undef YA_BITS_LOAD
#undef YA_BITS_PAIR
}

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V, bool GLOBAL_IDS,
    bool OFF32, bool DISTINCT = false, bool NEAR = false>
__device__ __forceinline__ void pass(const Entry<Pt>* __restrict__ sh_e, const float4* __restrict__ sh_v,
    Lds_word* const words,
    const int b0, const int e0, const int b1, const int e1, const int b2, const int e2,
    const int shift0, const int shift1, const int shift2, const float4* __restrict__ sorted_v,
    const Pt& Xi, const int i, const float cut2, Pt& F, float3& sum_v, float& sum_friction,
    const int* __restrict__ global_id, const int id_base = 0)
{
    const Scan sc = scan<Pt>(sh_e, words, b0, e0, b1, e1, b2, e2, Xi, cut2);
    drain<Pt, pw_int, pw_friction, STAGE_V, GLOBAL_IDS, OFF32, DISTINCT, NEAR>(sh_e, sh_v, words, sc, shift0, shift1,
        shift2, sorted_v, Xi, i, F, sum_v, sum_friction, global_id, id_base);
}
}  // namespace bits

// GLOBAL_IDS (z-slab decomposition): functors get global_id[local index]; a template parameter
// rather than a null test so that the single-GPU kernel carries neither the test nor the gather.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V, bool GLOBAL_IDS,
    bool OFF32>
__device__ __forceinline__ void grid_force_bits_tile(const int n, const int tile, const int id_base, const int half,
    const int slot, const Entry<Pt>* sorted, const float4* sorted_v,
    const int* cube_id, const int* offs, const int gs, const int n_cubes, const float cut2,
    Pt* d_dX, const bool has_gen, const int n_active, Pt* d_dX_sorted,
    const int* global_id, float* tail_exchange, int* tail_tickets, const bool by_plane, const int facts = 0);

// OFF32: old_v gathered through 32-bit byte offsets (bits::offsets_fit_32_bits(n); bits::pass)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V = false,
    bool GLOBAL_IDS = false, bool OFF32 = true>
__global__ __launch_bounds__(bits::BLOCK, bits::Min_waves<Pt>::value) void grid_force_bits(const int n,
    const Entry<Pt>* __restrict__ sorted, const float4* __restrict__ sorted_v,
    const int* __restrict__ cube_id, const int* __restrict__ offs, const int gs,
    const int n_cubes, const float cut2, Pt* __restrict__ d_dX, const bool has_gen,
    const int n_active, Pt* __restrict__ d_dX_sorted, const int* __restrict__ global_id, const int n_tiles,
    const int tail, float* tail_exchange, int* tail_tickets, const bool by_plane,
    const int part = 0, const int part_cube_lo = 0, const int part_cube_hi = 0, const int own_cube_lo = 0,
    const int own_cube_hi = 0x7fffffff, const int pass_facts = 0)
{
    constexpr int FB = bits::BLOCK;

    // z-slab decomposition: a stage's forces in two launches, so that the right-hand sides the
    // slab neighbours wait for are computed and sent first.  part 1 = the tiles that hold the
    // cells of the cubes below part_cube_lo or from part_cube_hi up (the z-planes next to the
    // slab's faces: cube ids are z-major, so these are the two ends of the sorted array), part 2
    // = the tiles in between, 0 = every tile.  Either launch spreads ITS tiles over all eight
    // XCDs (a launch that kept the whole array's mapping would occupy only the XCDs that own its
    // end of the array, and take as long as the full launch); blocks beyond its share exit.
    // Round 4: cubes below own_cube_lo and from own_cube_hi up hold mirrored cells only (the caller
    // knows how far own cells can have strayed): their tiles are not part of any launch.  And part 1
    // is dealt to the XCDs in SIXTEEN short ranges each instead of two: its list of tiles runs
    // mirrored cells -> own cells at the lower face and own -> mirrored at the upper one (a tile of
    // mirrored cells costs nothing), and with two ranges the XCDs in the middle of the list got
    // nearly twice the work of those at its ends -- all of them also carry an eighth of part 2.
    //
    // SUMMATION ORDER.  by_plane = false (Grid_computer::sum_order = YA_SUM_REFERENCE, the default): every
    // cell's terms go to ONE running sum over the nine rows in the reference's d_nhood order -- the
    // reference's arithmetic (solvers.cuh:437-459) -- and every tile is a whole tile (tail == 0).
    // by_plane = true (YA_SUM_BY_PLANE, a model's opt-in): S[dz = 0] + S[dz = -1, +1], which is what lets
    // THE TAIL exist (round 5): a launch ends with one wavefront lifetime at falling occupancy (16 % of a launch of
    // 10^6 cells).  The last `tail` tiles of a launch's list are then given to TWO one-wavefront
    // workgroups each -- half 0 the cells' own z-plane (~63 % of the pairs), half 1 the planes below and above
    // -- that live half as long and meet through memory: the half that finishes first leaves its sums in the
    // exchange area and draws the tile's ticket, the half that draws the second ticket adds the other's sums
    // to its own (a + b == b + a bit for bit) and stores the cells' right-hand sides.  A whole tile keeps the
    // own plane's sums aside and adds them at the end, so every cell's sums are S[dz = 0] + S[dz = -1, +1],
    // each in the reference's order from +0, whoever computed them: which tiles are split is a scheduling
    // decision without any effect on results (and the oracle sums in this order).  ONE launch, hardware
    // dispatch: blocks [0, whole) are whole tiles, blocks whole + 16 g + x and whole + 16 g + 8 + x the halves
    // of tile whole + 8 g + x, both on XCD x.  (Everything else that was tried to shorten the drain lost:
    // DESIGN.md section 6, round 5.)
    int tile, mine, t_first = 0, t_lo = 0, t_hi = 0;
    if (part == 0) {
        mine = n_tiles;
    } else {
        const int tiles = n_tiles;
        t_first = min(offs[min(max(own_cube_lo, 0), n_cubes)] / FB, tiles);
        const int t_end = max(min((offs[min(own_cube_hi, n_cubes)] + FB - 1) / FB, tiles), t_first);
        t_lo = max(min((offs[min(part_cube_lo, n_cubes)] + FB - 1) / FB, t_end), t_first);
        t_hi = max(min(offs[min(part_cube_hi, n_cubes)] / FB, t_end), t_lo);
        mine = part == 1 ? (t_lo - t_first) + (t_end - t_hi) : t_hi - t_lo;
    }
    // (tail < 0: EVERY tile as halves -- launches whose half tiles are all resident at once, where what
    // counts is not the drain but the lifetime itself)
    // (the two launches of a slab stage learn their list's length here, not on the host: a list of fewer than
    // four tails' tiles stays whole)
    const int whole = tail < 0 ? 0 : (tail > 0 && (part == 0 || mine >= 4 * tail) ? max(mine - tail, 0) & ~7 : mine);
    int half = -1, compact = blockIdx.x;
    if (compact >= whole) {
        const int b = compact - whole;
        half = (b >> 3) & 1;
        compact = whole + (b >> 4) * 8 + (b & 7);
    }
    if (compact >= mine) return;
    if (part == 0) {
        tile = xcd_contiguous_tile(compact, mine);
    } else {
        // (part 2 as well: in the cap of a ball -- the first and the last slab -- the tiles' cost falls
        // or rises all along the list, and two ranges per XCD, paired for a whole ball's rise and
        // fall, left the XCD with the two dearest ranges 10 % behind)
        const int t = xcd_contiguous_tile<16>(compact, mine);
        if (part == 1)
            tile = t < t_lo - t_first ? t_first + t : t_hi + (t - (t_lo - t_first));
        else
            tile = t_lo + t;
    }
    // which tile is mine ends here; the tile itself is the body an ensemble's kernel shares (include/ensemble_grid.cuh)
    grid_force_bits_tile<Pt, pw_int, pw_friction, STAGE_V, GLOBAL_IDS, OFF32>(n, tile, 0, half, compact - whole, sorted,
        sorted_v, cube_id, offs, gs, n_cubes, cut2, d_dX, has_gen, n_active, d_dX_sorted, global_id, tail_exchange,
        tail_tickets, by_plane, pass_facts);
}

// One tile of grid_force_bits -- 64 consecutive sorted slots of ONE system's arrays -- as the workgroup that was
// given it: half < 0 a whole tile, 0 / 1 one half of exchange slot `slot` ("the tail", above).  The functors are
// handed the ids id_base + id (an ensemble's replica starts at id_base and its cube ids and offs[] are its own, so
// the clamps of YA_ROW_BOUNDS keep every stencil row inside the replica's segment; a lone system's constant 0
// folds away).  (No __restrict__ here: what may alias is said once, by the kernels' own parameters.)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V, bool GLOBAL_IDS,
    bool OFF32>
__device__ __forceinline__ void grid_force_bits_tile(const int n, const int tile, const int id_base, const int half,
    const int slot, const Entry<Pt>* sorted, const float4* sorted_v,
    const int* cube_id, const int* offs, const int gs, const int n_cubes, const float cut2,
    Pt* d_dX, const bool has_gen, const int n_active, Pt* d_dX_sorted,
    const int* global_id, float* tail_exchange, int* tail_tickets, const bool by_plane, const int facts)
{
    constexpr int FB = bits::BLOCK;
    constexpr int CAP = bits::Stage<Pt>::value;
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;  // sums kept per cell: F (NF), friction * old_v (3), friction
    __shared__ __attribute__((aligned(16))) Entry<Pt> sh_e[CAP + 8];  // slack: whole groups are read
    __shared__ unsigned sh_m[(bits::WORDS + 1) * FB];                // [word][thread], one spare row
    // STAGE_V (small systems, Grid_computer::forces): old_v of the staged cells in LDS as well.
    // A launch that cannot fill the chip is one wavefront per SIMD and nothing hides the round
    // trip to L2 that every interacting pair's old_v otherwise costs.
    __shared__ float4 sh_v[STAGE_V ? CAP + 8 : 1];
    bits::Lds_word* const words = (bits::Lds_word*)sh_m + threadIdx.x;
    const int s0 = tile * FB;
    const int s = s0 + threadIdx.x;
    bool active = s < n;
    const int c_lo = cube_id[s0];
    const int c_hi = cube_id[min(s0 + FB, n) - 1];
    YA_BITS_PROBE_BEGIN

    Pt Xi = ya::zero<Pt>();
    int i = 0, c = c_lo;
    if (active) {
        const Entry<Pt> self = sorted[s];
        Xi = self.X;
        i = self.id;
        c = cube_id[s];
        active = i < n_active;  // ghost cells of a slab decomposition get no force
    }
    if (!__syncthreads_or(active)) return;  // a workgroup of ghosts only
    // functors see GLOBAL ids in a slab decomposition (they index per-cell model arrays)
    const int gi = (GLOBAL_IDS && active ? global_id[i] : i) + id_base;
    Pt F = ya::zero<Pt>();
    float3 sum_v{0.f, 0.f, 0.f};
    float sum_friction = 0;

    // a whole tile: the sums of the own plane while the other two planes are walked -- in registers for
    // three-float points (91 VGPRs: five wavefronts per SIMD as before), in a lane-private LDS column for
    // wider ones, whose functors leave no registers (relu_w_epithelium: 161 -> 172 VGPRs would cost the third
    // wavefront per SIMD)
    constexpr bool OWN_IN_LDS = sizeof(Pt) > 16;
    __shared__ float sh_own[OWN_IN_LDS ? NC * FB : 1];
    float own[OWN_IN_LDS ? 1 : NC];
#pragma unroll
    for (int k = 0; k < (OWN_IN_LDS ? 1 : NC); k++) own[k] = 0.f;

    int next_lo[3], next_hi[3], next_begin[3], next_end[3];
    const int plane_first = half == 1 ? 1 : 0, plane_end = half == 0 ? 1 : 3;
#pragma unroll 1
    for (int plane = plane_first; plane < plane_end; plane++) {
        if (by_plane && half < 0 && plane == 1) {
            float save[NC];
#pragma unroll
            for (int k = 0; k < NF; k++) save[k] = field(F, k);
            save[NF] = sum_v.x, save[NF + 1] = sum_v.y, save[NF + 2] = sum_v.z, save[NF + 3] = sum_friction;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                if (OWN_IN_LDS)
                    sh_own[k * FB + threadIdx.x] = save[k];
                else
                    own[OWN_IN_LDS ? 0 : k] = save[k];
            }
            F = ya::zero<Pt>(), sum_v = float3{0.f, 0.f, 0.f}, sum_friction = 0;
        }
        int wg_begin[3], v0[4], k_begin[3], k_end[3];
        v0[0] = 0;
        YA_ROW_BOUNDS(plane)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            wg_begin[r] = next_lo[r];
            v0[r + 1] = v0[r] + next_hi[r] - wg_begin[r];
            k_begin[r] = next_begin[r];
            k_end[r] = active ? next_end[r] : k_begin[r];
        }
        const int total = v0[3];

        for (int chunk = 0; chunk < total; chunk += CAP) {
            const int chunk_n = min(CAP, total - chunk);
            __syncthreads();
            for (int t = threadIdx.x; t < chunk_n; t += FB) {
                const int v = chunk + t;
                const int shift = v >= v0[2] ? wg_begin[2] - v0[2]
                                             : (v >= v0[1] ? wg_begin[1] - v0[1] : wg_begin[0]);
                sh_e[t] = sorted[v + shift];
                if (STAGE_V) sh_v[t] = sorted_v[v + shift];
            }
            __syncthreads();
            // this lane's candidates of the three rows, as LDS indices clipped to the chunk
            int sb[3], se[3], shift[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                sb[r] = max(k_begin[r] - wg_begin[r] + v0[r], chunk) - chunk;
                se[r] = min(k_end[r] - wg_begin[r] + v0[r], chunk + chunk_n) - chunk;
                shift[r] = wg_begin[r] - v0[r] + chunk;
            }
            const int bits_needed = (max(se[0] - sb[0], 0) + 3 & ~3) + (max(se[1] - sb[1], 0) + 3 & ~3) +
                                    (max(se[2] - sb[2], 0) + 3 & ~3);
            if (!__any(bits_needed > bits::PASS_BITS)) {
                const bits::Scan sc = bits::scan<Pt>(sh_e, words, sb[0], se[0], sb[1], se[1], sb[2], se[2], Xi, cut2);
                // phase 2 under what this pass knows about its hits (bits::FACT_DISTINCT, FACT_NEAR): the own slot is
                // looked for in the pass' candidate ranges themselves, never inferred from the plane
#define YA_BITS_DRAIN(distinct_, near_)                                                        \
    bits::drain<Pt, pw_int, pw_friction, STAGE_V, GLOBAL_IDS, OFF32, distinct_, near_>(sh_e, sh_v, words, sc, shift[0], \
        shift[1], shift[2], sorted_v, Xi, gi, F, sum_v, sum_friction, global_id, id_base)
                constexpr bool GENERIC_ONLY = GLOBAL_IDS || !bits::FACT_BODIES;  // slabs; the fast tier
                bool distinct = false;
                if constexpr (!GENERIC_ONLY) {
                    bool own_among = false;
#pragma unroll
                    for (int r = 0; r < 3; r++) own_among |= (s - shift[r] >= sb[r]) & (s - shift[r] < se[r]);
                    distinct = (facts & bits::FACT_DISTINCT) && !__any(own_among);
                }
                const bool near = facts & bits::FACT_NEAR;
                if constexpr (GENERIC_ONLY) {
                    YA_BITS_DRAIN(false, false);
                } else if (distinct) {
                    if (near)
                        YA_BITS_DRAIN(true, true);
                    else
                        YA_BITS_DRAIN(true, false);
                } else if (near) {
                    YA_BITS_DRAIN(false, true);
                } else {
                    YA_BITS_DRAIN(false, false);
                }
#undef YA_BITS_DRAIN
            } else {
                // dense rows: one pass per stretch of PASS_BITS candidates, rows in order
#pragma unroll 1
                for (int r = 0; r < 3; r++) {
                    const int rb = r == 0 ? sb[0] : (r == 1 ? sb[1] : sb[2]);
                    const int re = r == 0 ? se[0] : (r == 1 ? se[1] : se[2]);
                    const int rs = r == 0 ? shift[0] : (r == 1 ? shift[1] : shift[2]);
#pragma unroll 1
                    for (int b = rb; __any(b < re); b += bits::PASS_BITS)
                        bits::pass<Pt, pw_int, pw_friction, STAGE_V, GLOBAL_IDS, OFF32>(sh_e, sh_v, words, b, min(re, b + bits::PASS_BITS),
                            0, 0, 0, 0, rs, 0, 0, sorted_v, Xi, gi, cut2, F, sum_v, sum_friction, global_id, id_base);
                }
            }
        }
    }
    float sums[NC];
#pragma unroll
    for (int k = 0; k < NF; k++) sums[k] = field(F, k);
    sums[NF] = sum_v.x, sums[NF + 1] = sum_v.y, sums[NF + 2] = sum_v.z, sums[NF + 3] = sum_friction;
    if (half < 0) {
        if (by_plane) {
#pragma unroll
            for (int k = 0; k < NC; k++)  // S[dz = 0] + S[dz = -1, +1]
                sums[k] = (OWN_IN_LDS ? sh_own[k * FB + threadIdx.x] : own[OWN_IN_LDS ? 0 : k]) + sums[k];
        }
    } else {
        // INVARIANT the hand-over below relies on (not promised by the HIP memory model; guarded by
        // tests/test_parity_gpu.py::test_tail_exchange_over_many_launches): both halves of a tile run on ONE
        // XCD (blocks whole + 16 g + x and whole + 16 g + 8 + x: same x = blockIdx % 8), the sums are
        // stored with device-scope (sc1) relaxed atomics that go past that XCD's L2, and the ticket is drawn
        // only after `s_waitcnt vmcnt(0)` has seen every one of those stores acknowledged.
        // Device-scope relaxed atomic stores and loads (sc1) are performed past the XCD's L2, so no fence is
        // needed for the DATA (a device-scope release fence would write back the whole L2 once per workgroup:
        // 65 us per 1024 workgroups, core.hip's one-launch reduction).  What orders the sums before the ticket
        // is the explicit wait: the ticket is drawn only after every store of this wavefront has been
        // acknowledged at device scope (a workgroup-scope fence and the barrier compile to nothing in a
        // one-wavefront workgroup, and the stores and the atomic travel to different channels).
        __shared__ int sh_second;
        float* const mine_out = tail_exchange + ((size_t)slot * 2 + half) * NC * FB + threadIdx.x;
#pragma unroll
        for (int k = 0; k < NC; k++)
            __hip_atomic_store(mine_out + k * FB, sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0)
            sh_second = __hip_atomic_fetch_add(&tail_tickets[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (sh_second == 0) {  // the other half will finish the tile
            YA_BITS_PROBE_END(tile)
            return;
        }
        if (threadIdx.x == 0) __hip_atomic_store(&tail_tickets[slot], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float* const theirs = tail_exchange + ((size_t)slot * 2 + (1 - half)) * NC * FB + threadIdx.x;
#pragma unroll
        for (int k = 0; k < NC; k++)
            sums[k] = sums[k] + __hip_atomic_load(theirs + k * FB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (active) {
#pragma unroll
        for (int k = 0; k < NF; k++) field(F, k) = sums[k];
        const Pt dX = store_rhs(d_dX, i, has_gen, F, float3{sums[NF], sums[NF + 1], sums[NF + 2]}, sums[NF + 3]);
        if (d_dX_sorted) d_dX_sorted[s] = dX;  // for the sorted-space Euler stage
    }
    YA_BITS_PROBE_END(tile)
}


// ---------------------------------------------------------------------------------
// grid_force_coop (the solver's own choice below ~7 * 10^4 cells for functors declared YA_STATELESS;
// forced by Grid_computer::force_variant = 3): the grid force with SEVERAL LANES
// PER CELL, for systems too small to fill the chip with one lane per cell.  A launch of
// <= 10^5 cells is at most one wavefront per SIMD for the kernels above, each lane working
// through its ~265 candidates and ~41 hits alone: 52-65 us whatever n is.  Here a 256-thread
// workgroup owns 256 / LANES consecutive sorted slots (LANES = 16, 8 or 4, chosen from n).  All
// nine stencil rows are staged in LDS at once when they fit (they do at the densities models
// run at; otherwise plane by plane, in chunks), then for every cell
//
//   A  row by row in the reference's order, each of its lanes tests a contiguous share of the
//      row's candidates into a bit mask (as grid_force_bits does); a prefix sum of the lanes'
//      hit counts ranks the hits, which are left as one compact list per cell in LDS, still in
//      the reference's order;
//   B  LANES hits at a time, lane l evaluates hit l of the round (distance, functor,
//      friction) and leaves the pair's terms {F, friction, friction * old_v} in LDS;
//   C  ONE lane per component adds the round's terms to that component's sum in list order.
//
// Every per-cell sum is therefore accumulated in exactly the order of the kernels above (the reference's one
// running sum, or own plane | other planes under YA_SUM_BY_PLANE) and the result is bit-identical to theirs.  What changes is the same as for tile_force_coop: the
// functor is called for one i from several lanes at once, so functors that update per-cell
// state non-atomically (d_mes_nbs[i] += 1, examples/passive_growth.cu:48-51) must keep one
// lane per cell.  A, B and C of a cell run inside one wavefront: the only workgroup barriers
// are those around staging.
namespace coop {
constexpr int BLOCK = 256;
#ifndef YA_COOP_MAX_HITS
#define YA_COOP_MAX_HITS 96
#endif
constexpr int MAX_HITS = YA_COOP_MAX_HITS;  // hit-list length per cell; more hits are worked off in parts
constexpr int STRETCH = 64;   // candidates of a row ranked at a time (<= MAX_HITS, <= 32 per lane)
// staged cells: nine rows of (the workgroup's cells + two cubes) at rho ~ 10 per cube; wider
// entries go plane by plane unless the workgroup is 16 cells (branching model, 32-byte entries,
// 10^4 cells: 200 -> 171 us per step with all rows at once, but 3 * 10^4 with 8 lanes 212 -> 225)
template<typename Pt, int LANES>
struct Stage {
    static constexpr bool all_rows = sizeof(Entry<Pt>) <= 16 || (sizeof(Entry<Pt>) <= 32 && LANES == 16);
    static constexpr int value = (all_rows ? 9 : 5) * (BLOCK / LANES + 34);
};
// Lanes per cell for a launch of n cells (MI355X, springs at rho ~ 10, tools/micro/force_ab.hip:
// 16 lanes 19 us at 10^4 cells, 8 lanes 24 us at 3 * 10^4, 4 lanes 39 us at 6.5 * 10^4, where one lane
// per cell takes 53, 64 and 61 us); 1 = one lane per cell is as fast or faster -- since round 5 that is
// grid_force_bits with EVERY tile as two half-tile workgroups while all of them are resident at once
// (Grid_computer::forces): 53 us at 10^5 cells where 4 lanes take 58 (their 1250 workgroups no longer fit
// the chip in one round from 8 * 10^4 cells on), 63 at 1.5 * 10^5 where they take 79 and whole tiles 71.
// Under the default summation order (no half tiles) four lanes per cell stay ahead of whole tiles up to
// ~1.2 * 10^5 cells (10^5: 58 against 62 us; 1.5 * 10^5: 79 against 71).
inline int lanes_for(const int n, const bool by_plane = false)
{
    return n <= 15000 ? 16 : (n <= 40000 ? 8 : (n <= (by_plane ? 70000 : 120000) ? 4 : 1));
}
// LDS traffic between the lanes of ONE wavefront: the hardware keeps a wavefront's LDS
// operations in order, the compiler must too.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace coop

// The body, for ONE system's arrays: the workgroup is the system's `block`-th of `n_blocks` and owns 256 / LANES of
// its sorted slots; the functors are handed the ids id_base + id (grid_force_bits_tile's comment).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES>
__device__ __forceinline__ void grid_force_coop_cells(const int n, const int block, const int n_blocks,
    const int id_base, const Entry<Pt>* sorted, const float4* sorted_v,
    const int* cube_id, const int* offs, const int gs,
    const int n_cubes, const float cut2, Pt* d_dX, const bool has_gen,
    const int n_active, Pt* d_dX_sorted, const int* global_id, const bool by_plane)
{
    static_assert(LANES == 4 || LANES == 8 || LANES == 16, "lanes per cell");
    constexpr int CELLS = coop::BLOCK / LANES, MAX_HITS = coop::MAX_HITS;
    constexpr int CAP = coop::Stage<Pt, LANES>::value;
    static_assert(CAP < 4096, "a listed hit is row << 12 | LDS index");
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;  // components summed per cell: F (NF), friction, friction * old_v (3)
    constexpr int SLOTS = (NC + LANES - 1) / LANES;
    constexpr bool STAGE_V = LANES >= 8;  // old_v in LDS too where the launch is too small to hide L2
    __shared__ __attribute__((aligned(16))) Entry<Pt> sh_e[CAP + 4];  // slack: whole groups are read
    __shared__ float4 sh_v[STAGE_V ? CAP : 1];
    __shared__ unsigned short sh_hit[CELLS][MAX_HITS];  // row << 12 | LDS index of the hit
    __shared__ __attribute__((aligned(16))) float sh_term[CELLS][NC][LANES];  // one round's terms
    __shared__ float sh_sum[CELLS][NC];
    // row r of the stencil: the workgroup's slot range is [sh_lo[r], sh_lo[r] + sh_len[r]);
    // a cell's own candidates are the slots [sh_kb[cell][r], sh_ke[cell][r])
    __shared__ int sh_lo[9], sh_len[9], sh_shift[9], sh_kb[CELLS][9], sh_ke[CELLS][9];

    const int cell = threadIdx.x / LANES, lane = threadIdx.x % LANES;
    const int s0 = xcd_contiguous_tile(block, n_blocks) * CELLS;
    const int s = s0 + cell;
    bool active = s < n;

    Pt Xi = ya::zero<Pt>();
    int i = 0, c = 0;
    if (active) {
        const Entry<Pt> self = sorted[s];
        Xi = self.X;
        i = self.id;
        c = cube_id[s];
        active = i < n_active;  // ghost cells of a slab decomposition get no force
    }
    if (!__syncthreads_or(active)) return;  // a workgroup of ghosts only
    const int gi = (global_id && active ? global_id[i] : i) + id_base;
    // The reference indexes cube_start/end without bounds checks (solvers.cuh:444);
    // out-of-grid cubes are treated as empty here.
    for (int r = lane; r < 9; r += LANES) {
        const int off = stencil_row_offset(r, gs);
        const int begin = offs[min(max(c + off - 1, 0), n_cubes)];
        sh_kb[cell][r] = begin;
        sh_ke[cell][r] = active ? offs[min(max(c + off + 2, 0), n_cubes)] : begin;
    }
    if (threadIdx.x < 9) {
        const int off = stencil_row_offset(threadIdx.x, gs);
        const int c_lo = cube_id[s0], c_hi = cube_id[min(s0 + CELLS, n) - 1];
        const int lo = offs[min(max(c_lo + off - 1, 0), n_cubes)];
        sh_lo[threadIdx.x] = lo;
        sh_len[threadIdx.x] = offs[min(max(c_hi + off + 2, 0), n_cubes)] - lo;
    }
    __syncthreads();
    int v0[10];  // row r sits at [v0[r], v0[r + 1]) of the nine ranges laid end to end
    v0[0] = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) v0[r + 1] = v0[r] + sh_len[r];
    if (threadIdx.x < 9) {
        int mine = 0;
#pragma unroll
        for (int r = 0; r < 9; r++) mine = (int)threadIdx.x == r ? v0[r] : mine;
        sh_shift[threadIdx.x] = sh_lo[threadIdx.x] - mine;  // position in the nine ranges -> sorted slot
    }
    __syncthreads();

    float acc[SLOTS];  // this lane's component sums (components lane, lane + LANES, ...)
    // by_plane (Grid_computer::sum_order = YA_SUM_BY_PLANE; grid_force_bits, "the tail"): the own plane's sums
    // (rows 0-2) are kept aside and the other planes' summed from +0; the two are added at the end.  A cell's
    // hit list never mixes the two: listing stops before row 3 until the own plane's list has been worked off.
    // Otherwise (the default, the reference's order) one running sum: own_done from the start, acc_own stays +0
    // (and +0 + x is x for every x a sum that started at +0 can hold: never -0).
    float acc_own[SLOTS];
#pragma unroll
    for (int a = 0; a < SLOTS; a++) acc[a] = 0.f, acc_own[a] = 0.f;
    bool own_done = !by_plane;
#define YA_COOP_OWN_DONE                                          \
    {                                                             \
        _Pragma("unroll") for (int a = 0; a < SLOTS; a++) acc_own[a] = acc[a], acc[a] = 0.f; \
        own_done = true;                                          \
    }

    const int rows_at_once = v0[9] <= CAP ? 9 : 3;
#pragma unroll 1
    for (int g0 = 0; g0 < 9; g0 += rows_at_once) {
        const int g_end = g0 + rows_at_once;
        if (g0 == 3 && !own_done) YA_COOP_OWN_DONE  // plane by plane: every list is worked off at the end of a chunk
        const int g_base = g0 == 0 ? 0 : (g0 == 3 ? v0[3] : v0[6]);
        const int g_total = (g_end == 9 ? v0[9] : (g_end == 3 ? v0[3] : v0[6])) - g_base;
#pragma unroll 1
        for (int chunk = 0; chunk < g_total; chunk += CAP) {
            const int chunk_n = min(CAP, g_total - chunk);
            const int base = g_base + chunk;  // where sh_e[0] sits in the nine ranges laid end to end
            __syncthreads();
            for (int t = threadIdx.x; t < chunk_n; t += coop::BLOCK) {
                const int v = base + t;
                int r = 0;
#pragma unroll
                for (int q = 1; q < 9; q++) r += v >= v0[q];
                const int slot = v + sh_shift[r];
                sh_e[t] = sorted[slot];
                if (STAGE_V) sh_v[t] = sorted_v[slot];
            }
            __syncthreads();

            // the cell's candidates of row r inside this chunk: LDS indices [sb, sb + len);
            // the next row's are requested while this one is worked on
            int r = g0, sb, len, k0 = 0, sb_next, len_next;
#define YA_COOP_ROW(row_, sb_, len_)                                                   \
    {                                                                                  \
        const int rr = min(row_, 8);                                                   \
        const int shift = sh_shift[rr] + base;                                         \
        sb_ = max(sh_kb[cell][rr] - shift, 0);                                         \
        len_ = (row_) < g_end ? max(min(sh_ke[cell][rr] - shift, chunk_n) - sb_, 0) : 0; \
    }
            YA_COOP_ROW(g0, sb, len)
            YA_COOP_ROW(g0 + 1, sb_next, len_next)
            int listed = 0;  // hits in the cell's list (the same in all its lanes)
            while (true) {
                // ---- A: stretches of rows until every cell of the wavefront is through or
                // its list could overflow ----
                while (true) {
                    const int row_limit = own_done ? g_end : min(g_end, 3);
                    const int stretch = r < row_limit ? min(len - k0, coop::STRETCH) : 0;
                    const bool go = r < row_limit && listed + stretch <= MAX_HITS;
                    if (!__any(go)) break;
                    if (go) {
                        // this lane's share [pb, pe) of the stretch: bit j of the mask, counted
                        // from the top, is candidate pb + j
                        const int share = (stretch + LANES - 1) / LANES;
                        const int pb = sb + k0 + min(lane * share, stretch);
                        const int pe = sb + k0 + min(lane * share + share, stretch);
                        unsigned m = 0;
                        int bits = 0;
                        for (int t = pb; t < pe; t += 4) {
                            float4 w[4];
                            float d2[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) w[u] = staged_words(&sh_e[t + u]);
#pragma unroll
                            for (int u = 0; u < 4; u++) {
                                d2[u] = dist2_to(Xi, w[u]);
                                keep_wide(w[u]);
                                d2[u] = t + u < pe ? d2[u] : INFINITY;
                            }
#pragma unroll
                            for (int u = 0; u < 4; u++) bits::shift_in(m, d2[u], cut2);
                            bits += 4;
                        }
                        m = bits > 0 ? m << (32 - bits) : 0u;
                        const int mine = __builtin_popcount(m);
                        int upto = mine;  // hits of this lane and of the cell's lower lanes
#pragma unroll
                        for (int o = 1; o < LANES; o <<= 1) {
                            const int up = __shfl_up(upto, o, LANES);
                            upto += lane >= o ? up : 0;
                        }
                        int rank = listed + upto - mine;
                        listed += __shfl(upto, LANES - 1, LANES);
                        while (m != 0) {
                            const int pos = __builtin_clz(m);
                            m &= 0x7fffffffu >> pos;
                            sh_hit[cell][rank++] = (unsigned short)((r << 12) | (pb + pos));
                        }
                        k0 += stretch;
                        while (k0 >= len && r < g_end) {
                            r++;
                            k0 = 0;
                            sb = sb_next;
                            len = len_next;
                            YA_COOP_ROW(r + 1, sb_next, len_next)
                        }
                    }
                }
                if (!__any(listed > 0)) {
                    if (!__any(r < g_end)) break;  // every cell is through all rows
                    if (rows_at_once == 9 && !own_done && r >= 3) YA_COOP_OWN_DONE  // no hit in the own plane's last rows
                    continue;
                }
                coop::wave_sync();
                // ---- B and C, LANES hits per round.  Lanes past the end of the list leave zero
                // terms: a sum that starts at +0 never is -0, so adding +0 changes no bit ----
                for (int h0 = 0; __any(h0 < listed); h0 += LANES) {
                    const int h = h0 + lane;
                    Pt f = ya::zero<Pt>();
                    float friction = 0;
                    float4 v{0.f, 0.f, 0.f, 0.f};
                    if (h < listed) {
                        const int e = sh_hit[cell][h];
                        const int t = e & 0xfff;
                        const Entry<Pt> other = sh_e[t];
                        if (STAGE_V)
                            v = sh_v[t];
                        else
                            v = sorted_v[(unsigned)(t + base + sh_shift[e >> 12])];
                        Pt rr = Xi - other.X;
                        float dist = dist3(rr.x, rr.y, rr.z);
                        const int j = (global_id ? global_id[other.id] : other.id) + id_base;
                        YA_CALL_INLINED f = pw_int(Xi, rr, dist, gi, j);
                        friction = pw_friction(Xi, rr, dist, gi, j);
                    }
#pragma unroll
                    for (int q = 0; q < NF; q++) sh_term[cell][q][lane] = field(f, q);
                    sh_term[cell][NF][lane] = friction;
                    // the old_v term only where the friction is not zero (solvers.cuh:454-458)
                    sh_term[cell][NF + 1][lane] = friction != 0 ? friction * v.x : 0.f;
                    sh_term[cell][NF + 2][lane] = friction != 0 ? friction * v.y : 0.f;
                    sh_term[cell][NF + 3][lane] = friction != 0 ? friction * v.z : 0.f;
                    coop::wave_sync();
#pragma unroll
                    for (int a = 0; a < SLOTS; a++) {
                        const int q = lane + LANES * a;
                        if (q < NC) {
                            float sum = acc[a];
                            const float4* terms = reinterpret_cast<const float4*>(&sh_term[cell][q][0]);
#pragma unroll
                            for (int u = 0; u < LANES / 4; u++) {
                                const float4 p = terms[u];
                                sum += p.x;
                                sum += p.y;
                                sum += p.z;
                                sum += p.w;
                            }
                            acc[a] = sum;
                        }
                    }
                    coop::wave_sync();
                }
                listed = 0;
                if (rows_at_once == 9 && !own_done && r >= 3) YA_COOP_OWN_DONE
            }
#undef YA_COOP_ROW
        }
    }
#pragma unroll
    for (int a = 0; a < SLOTS; a++) {
        const int q = lane + LANES * a;
        if (q < NC) sh_sum[cell][q] = acc_own[a] + acc[a];
    }
#undef YA_COOP_OWN_DONE
    coop::wave_sync();
    if (active && lane == 0) {
        Pt F;
#pragma unroll
        for (int q = 0; q < NF; q++) field(F, q) = sh_sum[cell][q];
        const Pt dX = store_rhs(d_dX, i, has_gen, F,
            float3{sh_sum[cell][NF + 1], sh_sum[cell][NF + 2], sh_sum[cell][NF + 3]}, sh_sum[cell][NF]);
        if (d_dX_sorted) d_dX_sorted[s] = dX;  // for the sorted-space Euler stage
    }
}

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES>
__global__ __launch_bounds__(coop::BLOCK) void grid_force_coop(const int n,
    const Entry<Pt>* __restrict__ sorted, const float4* __restrict__ sorted_v,
    const int* __restrict__ cube_id, const int* __restrict__ offs, const int gs,
    const int n_cubes, const float cut2, Pt* __restrict__ d_dX, const bool has_gen,
    const int n_active, Pt* __restrict__ d_dX_sorted, const int* __restrict__ global_id, const bool by_plane)
{
    grid_force_coop_cells<Pt, pw_int, pw_friction, LANES>(n, blockIdx.x, gridDim.x, 0, sorted, sorted_v, cube_id, offs,
        gs, n_cubes, cut2, d_dX, has_gen, n_active, d_dX_sorted, global_id, by_plane);
}

#undef YA_ROW_BOUNDS

// Gabriel-graph force (replaces compute_cube_gabriel, solvers.cuh:509-602).  The reference's thread, per
// cell i: (1) collect every cell of the 27 cubes with dist < cube_size, the cell itself included, in
// d_nhood order and grid order inside a cube; (2) order them by distance with its selection sort (strict
// `<`, swaps: NOT stable); (3) from the farthest to the closest candidate m, drop the pair (i, j) if a
// candidate q < m lies strictly inside the sphere around the midpoint of i and j with radius
// 0.5f * dist * coefficient (never for j == i); (4) add the kept pairs' terms in that same order.
//
// Here GABRIEL_LANES lanes share a cell (GABRIEL_CELLS cells per one-wavefront workgroup):
//   scan     the lanes stream the 9 stencil rows of the sorted arrays and compact the hits into the cell's
//            LDS list in candidate order (ballot + popcount of the lower lanes' bits);
//   rank     each lane ranks its own candidates: rank = #closer + #equally close earlier in the list.  With
//            all distances distinct (and none NaN) the selection sort's permutation IS that ascending
//            order, whatever the start order.  Where a cell has a tie (lattices are full of them) or a NaN,
//            one lane runs the reference's selection sort itself on the LDS list: ties change the order of
//            the sum, hence its bits (tests/test_gabriel_*.py hold both paths bit for bit);
//   test     each lane tests its own candidates against those ranked before them -- and, for functors
//            declared stateless (YA_STATELESS), evaluates the terms of the pairs it keeps;
//   sum      one lane adds the kept pairs' terms (evaluating them itself for other functors: per-cell
//            counters like `d_n_nbs[i] += 1` see one lane, in order), farthest first, as the reference does.
// No private arrays (0 bytes of scratch).  A cell with more than GABRIEL_CAP candidates is not done here:
// it is appended to a list, and ya::gabriel_force_dense does it with a global workspace (Gabriel_computer
// sizes it from the counted candidates), so any number of candidates is right and in bounds.
constexpr int GABRIEL_LANES = 16;
constexpr int GABRIEL_CELLS = 64 / GABRIEL_LANES;
constexpr int GABRIEL_CAP = 64;  // candidates of a cell the LDS list holds (~13 at random_sphere(0.75), ~41 at the springs state)
constexpr int GABRIEL_DENSE_ARRAYS = 8;  // x, y, z, d, slot, rank, order, kept: the dense kernel's lists

namespace gabriel {
// The reference's selection sort (solvers.cuh:550-566) of the list's indices by distance, one lane.
template<typename Index>
__device__ __forceinline__ void selection_sort(const int count, const float* d, Index* order)
{
    for (int m = 0; m < count; m++) order[m] = (Index)m;
    for (int m = 0; m < count - 1; m++) {
        float min_val = d[order[m]];
        int min_index = m;
        for (int q = m + 1; q < count; q++) {
            const float compare_val = d[order[q]];
            if (compare_val < min_val) {
                min_index = q;
                min_val = compare_val;
            }
        }
        if (min_index != m) {
            const Index t = order[min_index];
            order[min_index] = order[m];
            order[m] = t;
        }
    }
}
// Is a candidate ranked below `rank` strictly inside the sphere (mx, my, mz; radius)?  (solvers.cuh:584-592:
// the reference walks them from rank - 1 down and stops at the first; which one it finds does not matter.)
template<typename Index>
__device__ __forceinline__ bool occluded(const int rank, const float mx, const float my, const float mz,
    const float radius, const Index* order, const float* x, const float* y, const float* z)
{
    for (int m = rank - 1; m >= 0; m--) {
        const int q = order[m];
        if (dist3(mx - x[q], my - y[q], mz - z[q]) < radius) return true;
    }
    return false;
}
// WHERE THE STAGES FIND THE CUBE-SORTED CELLS.  The stages below read a system's cells through `rows`: entry(k) = the
// cell in sorted slot k (position and id), X(k) its position alone, v(k) its old_v, cube(k) its cube,
// first_slot(c) = offs[c], c in [0, n_cubes].  Sorted_rows is a build's global arrays (every kernel of this file);
// ya::ens::Lds_rows (include/ensemble_gabriel.cuh) a replica's keys and step arrays in LDS.
template<typename Pt>
struct Sorted_rows {
    const Entry<Pt>* __restrict__ sorted;
    const float4* __restrict__ sorted_v;
    const int* __restrict__ cube_id;
    const int* __restrict__ offs;
    __device__ __forceinline__ Entry<Pt> entry(const int k) const { return sorted[k]; }
    __device__ __forceinline__ Pt X(const int k) const { return sorted[k].X; }
    __device__ __forceinline__ float4 v(const int k) const { return sorted_v[k]; }
    __device__ __forceinline__ int cube(const int k) const { return cube_id[k]; }
    __device__ __forceinline__ int first_slot(const int c) const { return offs[c]; }
};
// A cell's candidates into the list (x, y, z, d, slot) in the reference's order, by the `lanes` lanes
// from `first_lane` of the wavefront; returns the number of candidates (entries beyond cap are not written).
template<typename Pt, typename Rows>
__device__ __forceinline__ int collect(const int lane, const int lanes, const int first_lane, const Pt Xi,
    const int c, const Rows& rows, const int gs,
    const int n_cubes, const float cube_size, const int cap, float* x, float* y, float* z, float* d, int* slot)
{
    const unsigned long long group = (lanes == 64 ? ~0ull : ((1ull << lanes) - 1)) << first_lane;
    const unsigned long long below = group & ((1ull << (first_lane + lane)) - 1);
    int count = 0;
    for (int row = 0; row < 9; row++) {
        const int mid = c + stencil_row_offset(row, gs);
        const int k_begin = rows.first_slot(min(max(mid - 1, 0), n_cubes));
        const int k_end = rows.first_slot(min(max(mid + 2, 0), n_cubes));
        for (int base = k_begin; base < k_end; base += lanes) {
            const int k = base + lane;
            bool hit = false;
            Pt Xk;
            float dist = 0;
            if (k < k_end) {
                Xk = rows.X(k);
                const Pt r = Xi - Xk;
                dist = dist3(r.x, r.y, r.z);
                hit = !(dist >= cube_size);  // (solvers.cuh:540: a NaN distance is a candidate)
            }
            const unsigned long long hits = __ballot(hit) & group;
            if (hit) {
                const int q = count + __popcll(hits & below);
                if (q < cap) {
                    x[q] = Xk.x;
                    y[q] = Xk.y;
                    z[q] = Xk.z;
                    d[q] = dist;
                    slot[q] = k;
                }
            }
            count += __popcll(hits);
        }
    }
    return count;
}
// rank[p] = the place of candidate p in the selection sort's order, order[rank] = p: ranked by the lanes
// while the cell's distances are distinct, sorted by its first lane where they are not.
template<typename Index>
__device__ __forceinline__ void rank_list(const int lane, const int lanes, const int first_lane,
    const int count, const float* d, Index* rank, Index* order)
{
    const unsigned long long group = (lanes == 64 ? ~0ull : ((1ull << lanes) - 1)) << first_lane;
    bool odd = false;
    for (int p = lane; p < count; p += lanes) {
        const float dp = d[p];
        int r = 0;
        for (int q = 0; q < count; q++) {
            const float dq = d[q];
            r += (dq < dp || (dq == dp && q < p)) ? 1 : 0;
            odd |= dq == dp && q != p;
        }
        odd |= dp != dp;
        rank[p] = (Index)r;
    }
    const bool tied = (__ballot(odd) & group) != 0;
    coop::wave_sync();
    if (!tied) {
        for (int p = lane; p < count; p += lanes) order[rank[p]] = (Index)p;
    } else if (lane == 0) {
        selection_sort(count, d, order);
        for (int m = 0; m < count; m++) rank[order[m]] = (Index)m;
    }
    coop::wave_sync();
}

// The test and the sum of a cell whose list is ranked: kept[rank] by the lanes, then the kept pairs' terms
// in one lane, farthest first (the functors are called for i from that lane alone, in the reference's order:
// functors that count per cell, `d_n_nbs[i] += 1` of tests/test_solvers.cu:343-352, stay right).
// i and the sorted entries' ids are rows of d_dX; the functors are handed id_base + id (an ensemble's replica
// starts at id_base, include/ensemble_gabriel.cuh; a lone system's constant 0 folds away).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Index, typename Rows>
__device__ __forceinline__ void test_and_sum(const int lane, const int lanes, const int s, const Pt Xi,
    const int i, const int id_base, const int count, const float gabriel_coefficient, const float* x, const float* y,
    const float* z, const float* d, const int* slot, const Index* rank, const Index* order, Index* kept,
    const Rows& rows, Pt* __restrict__ d_dX,
    const bool has_gen)
{
    for (int p = lane; p < count; p += lanes) {  // solvers.cuh:575-593
        bool keep = true;
        if (slot[p] != s) {  // j != i
            const float radius = 0.5f * d[p] * gabriel_coefficient;
            keep = !occluded((int)rank[p], 0.5f * (Xi.x + x[p]), 0.5f * (Xi.y + y[p]), 0.5f * (Xi.z + z[p]),
                radius, order, x, y, z);
        }
        kept[rank[p]] = keep ? 1 : 0;
    }
    __threadfence_block();  // (the dense kernel's lists are in global memory)
    coop::wave_sync();
    if (lane != 0) return;
    Pt F = ya::zero<Pt>();  // solvers.cuh:594-599
    float3 sum_v{0.f, 0.f, 0.f};
    float sum_friction = 0;
    for (int m = count - 1; m >= 0; m--) {
        if (!kept[m]) continue;
        const int p = order[m];
        const float dist = d[p];
        const Entry<Pt> other = rows.entry(slot[p]);
        const Pt r = Xi - other.X;
        F += pw_int(Xi, r, dist, id_base + i, id_base + other.id);
        const float friction = pw_friction(Xi, r, dist, id_base + i, id_base + other.id);
        sum_friction += friction;
        // the old_v term only where the friction is not zero: the same bits as the reference's
        // unconditional `sum_v += friction * d_old_v[j]` unless old_v is not finite (0 * inf)
        if (friction != 0) {
            const float4 v = rows.v(slot[p]);
            sum_v.x += friction * v.x;
            sum_v.y += friction * v.y;
            sum_v.z += friction * v.z;
        }
    }
    store_rhs(d_dX, i, has_gen, F, sum_v, sum_friction);
}
// One cell, sorted slot s, by its group of GABRIEL_LANES lanes (lane of the group, whose first lane is first_lane of
// the wavefront): collect, rank, test, sum -- gabriel_force's stages, this file's comment above -- on the group's
// lists: `list` = GABRIEL_CAP floats for each of x, y, z, d while the list is tested, then, for stateless functors,
// for each of the NF + 4 terms of the kept pairs by rank (F, friction, friction * old_v); `slot` = GABRIEL_CAP ints;
// `ranks` = GABRIEL_CAP bytes each of rank, order, kept.  The right-hand side goes to d_dX[the cell's id] by store_rhs,
// the functors are handed id_base + id.  A cell with more than GABRIEL_CAP candidates is not done here: every lane of
// the group calls left_to_dense(count) and leaves, with nothing written to d_dX, and the caller sees that
// gabriel_force_dense_cell does the cell.  Lanes leave at different points: the caller's next statement is reached by
// all of them, and only wave_syncs lie in here.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Rows,
    typename Left_to_dense>
__device__ __forceinline__ void cell_by_group(const int lane, const int first_lane, const int s, const int id_base,
    const Rows& rows, const int gs, const int n_cubes, const float cube_size, const float gabriel_coefficient,
    float (*list)[GABRIEL_CAP], int* slot, unsigned char (*ranks)[GABRIEL_CAP], Pt* __restrict__ d_dX,
    const bool has_gen, const Left_to_dense& left_to_dense)
{
    constexpr int NF = N_floats<Pt>::value;
    constexpr int CAP = GABRIEL_CAP;
    constexpr int SLOTS = CAP / GABRIEL_LANES;
    float* x = list[0];
    float* y = list[1];
    float* z = list[2];
    float* d = list[3];
    unsigned char* rank = ranks[0];
    unsigned char* order = ranks[1];
    unsigned char* kept = ranks[2];
    const Entry<Pt> self = rows.entry(s);
    const Pt Xi = self.X;
    const int i = self.id;
    const int count = gabriel::collect(lane, GABRIEL_LANES, first_lane, Xi, rows.cube(s), rows, gs,
        n_cubes, cube_size, CAP, x, y, z, d, slot);
    if (count > CAP) {
        left_to_dense(count);
        return;
    }
    coop::wave_sync();
    gabriel::rank_list(lane, GABRIEL_LANES, first_lane, count, d, rank, order);
    if constexpr (!stateless_pair<Pt, pw_int, pw_friction>()) {
        gabriel::test_and_sum<Pt, pw_int, pw_friction>(lane, GABRIEL_LANES, s, Xi, i, id_base, count,
            gabriel_coefficient, x, y, z, d, slot, rank, order, kept, rows, d_dX, has_gen);
        return;
    } else {
        // Functors declared stateless (YA_STATELESS): each lane also evaluates the terms of the pairs it keeps
        // (into the position arrays, free once every lane has tested), and one lane only adds them up.
        bool keep[SLOTS];
        float dist[SLOTS];
        int rk[SLOTS], k[SLOTS];
#pragma unroll
        for (int a = 0; a < SLOTS; a++) {  // solvers.cuh:575-593, candidates p = lane + GABRIEL_LANES * a
            const int p = lane + GABRIEL_LANES * a;
            keep[a] = false;
            if (p < count) {
                dist[a] = d[p];
                rk[a] = rank[p];
                k[a] = slot[p];
                keep[a] = true;
                if (k[a] != s) {  // j != i
                    const float radius = 0.5f * dist[a] * gabriel_coefficient;
                    keep[a] = !gabriel::occluded(rk[a], 0.5f * (Xi.x + x[p]), 0.5f * (Xi.y + y[p]),
                        0.5f * (Xi.z + z[p]), radius, order, x, y, z);
                }
            }
        }
        coop::wave_sync();
#pragma unroll
        for (int a = 0; a < SLOTS; a++) {
            const int p = lane + GABRIEL_LANES * a;
            if (p >= count) continue;
            kept[rk[a]] = keep[a];
            if (!keep[a]) continue;
            const Entry<Pt> other = rows.entry(k[a]);
            const Pt r = Xi - other.X;
            const Pt F = pw_int(Xi, r, dist[a], id_base + i, id_base + other.id);
            const float friction = pw_friction(Xi, r, dist[a], id_base + i, id_base + other.id);
#pragma unroll
            for (int q = 0; q < NF; q++) list[q][rk[a]] = field(F, q);
            list[NF][rk[a]] = friction;
            if (friction != 0) {  // (see test_and_sum)
                const float4 v = rows.v(k[a]);
                list[NF + 1][rk[a]] = friction * v.x;
                list[NF + 2][rk[a]] = friction * v.y;
                list[NF + 3][rk[a]] = friction * v.z;
            }
        }
        coop::wave_sync();
        if (lane != 0) return;
        Pt F = ya::zero<Pt>();  // solvers.cuh:594-599
        float3 sum_v{0.f, 0.f, 0.f};
        float sum_friction = 0;
        for (int m = count - 1; m >= 0; m--) {
            if (!kept[m]) continue;
            Pt term;
#pragma unroll
            for (int q = 0; q < NF; q++) field(term, q) = list[q][m];
            F += term;
            const float friction = list[NF][m];
            sum_friction += friction;
            if (friction != 0) {
                sum_v.x += list[NF + 1][m];
                sum_v.y += list[NF + 2][m];
                sum_v.z += list[NF + 3][m];
            }
        }
        store_rhs(d_dX, i, has_gen, F, sum_v, sum_friction);
        return;
    }
}
}  // namespace gabriel

// ya::gabriel_force's workgroup over ONE system's arrays: the GABRIEL_CELLS sorted slots from `first_slot`, each by
// gabriel::cell_by_group on lists in static LDS.  The functors are handed the ids id_base + id, and a cell left to
// the dense kernel is appended as dense_base + its slot (an ensemble's replica starts at row id_base = dense_base of
// the flat arrays and its cube ids and offs[] are its own, include/ensemble_gabriel.cuh; a lone system's constant 0
// folds away).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__device__ __forceinline__ void gabriel_force_cells(const int n, const int first_slot, const int id_base,
    const int dense_base, const Entry<Pt>* __restrict__ sorted, const float4* __restrict__ sorted_v,
    const int* __restrict__ cube_id, const int* __restrict__ offs, const int gs,
    const int n_cubes, const float cube_size, const float gabriel_coefficient,
    Pt* __restrict__ d_dX, const bool has_gen, int* __restrict__ dense, int* __restrict__ n_dense)
{
    constexpr int NF = N_floats<Pt>::value;
    constexpr int CAP = GABRIEL_CAP;
    // x, y, z, d while the list is tested; then, for stateless functors, the kept pairs' terms by rank:
    // F (NF floats), friction, friction * old_v (3)
    constexpr int WORDS = NF + 4;
    __shared__ float sh_list[GABRIEL_CELLS][WORDS][CAP];
    __shared__ int sh_slot[GABRIEL_CELLS][CAP];
    __shared__ unsigned char sh_rank[GABRIEL_CELLS][3][CAP];  // rank, order, kept

    const int cell = threadIdx.x / GABRIEL_LANES;
    const int lane = threadIdx.x % GABRIEL_LANES;
    const int s = first_slot + cell;
    if (s >= n) return;  // (whole groups leave: everything below is per group)

    const gabriel::Sorted_rows<Pt> rows{sorted, sorted_v, cube_id, offs};
    gabriel::cell_by_group<Pt, pw_int, pw_friction>(lane, cell * GABRIEL_LANES, s, id_base, rows, gs, n_cubes, cube_size,
        gabriel_coefficient, sh_list[cell], sh_slot[cell], sh_rank[cell], d_dX, has_gen, [&](const int count) {
            if (lane == 0) {  // ya::gabriel_force_dense does this cell
                const int at = atomicAdd(&n_dense[0], 1);
                dense[at] = dense_base + s;
                atomicMax(&n_dense[1], count);
            }
        });
}

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force(const int n,
    const Entry<Pt>* __restrict__ sorted, const float4* __restrict__ sorted_v,
    const int* __restrict__ cube_id, const int* __restrict__ offs, const int gs,
    const int n_cubes, const float cube_size, const float gabriel_coefficient,
    Pt* __restrict__ d_dX, const bool has_gen, int* __restrict__ dense, int* __restrict__ n_dense)
{
    gabriel_force_cells<Pt, pw_int, pw_friction>(n, blockIdx.x * GABRIEL_CELLS, 0, 0, sorted, sorted_v, cube_id, offs,
        gs, n_cubes, cube_size, gabriel_coefficient, d_dX, has_gen, dense, n_dense);
}

// One cell ya::gabriel_force left (more than GABRIEL_CAP candidates), by one wavefront: the same stages on
// lists of `stride` >= the cell's count entries each, from x on (global memory here; LDS in
// ya::ens::gabriel_lds_steps).  s is the cell's sorted slot in ONE system's `rows`, the functors are handed
// id_base + id (gabriel_force_cells' comment).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Rows>
__device__ __forceinline__ void gabriel_force_dense_cell(const int lane, const int s, const int id_base,
    const Rows& rows, const int gs, const int n_cubes, const float cube_size,
    const float gabriel_coefficient, Pt* __restrict__ d_dX, const bool has_gen, float* x, const long stride)
{
    float* y = x + stride;
    float* z = y + stride;
    float* d = z + stride;
    int* slot = reinterpret_cast<int*>(d + stride);
    int* rank = slot + stride;
    int* order = rank + stride;
    int* kept = order + stride;
    const Entry<Pt> self = rows.entry(s);
    const Pt Xi = self.X;
    const int count = gabriel::collect(lane, 64, 0, Xi, rows.cube(s), rows, gs, n_cubes, cube_size,
        (int)stride, x, y, z, d, slot);
    __threadfence_block();
    coop::wave_sync();
    gabriel::rank_list(lane, 64, 0, count, d, rank, order);
    __threadfence_block();
    coop::wave_sync();
    gabriel::test_and_sum<Pt, pw_int, pw_friction>(lane, 64, s, Xi, self.id, id_base, count, gabriel_coefficient, x,
        y, z, d, slot, rank, order, kept, rows, d_dX, has_gen);
    __threadfence_block();
    coop::wave_sync();  // the next cell reuses the workspace
}
// (the global arrays of a build)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__device__ __forceinline__ void gabriel_force_dense_cell(const int lane, const int s, const int id_base,
    const Entry<Pt>* __restrict__ sorted, const float4* __restrict__ sorted_v, const int* __restrict__ cube_id,
    const int* __restrict__ offs, const int gs, const int n_cubes, const float cube_size,
    const float gabriel_coefficient, Pt* __restrict__ d_dX, const bool has_gen, float* x, const long stride)
{
    gabriel_force_dense_cell<Pt, pw_int, pw_friction>(lane, s, id_base,
        gabriel::Sorted_rows<Pt>{sorted, sorted_v, cube_id, offs}, gs, n_cubes, cube_size, gabriel_coefficient, d_dX,
        has_gen, x, stride);
}

// The cells ya::gabriel_force left: one wavefront per cell, lists in a global workspace of `stride` >= the
// largest count entries each, per workgroup.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force_dense(const int* __restrict__ dense,
    const int* __restrict__ n_dense, const Entry<Pt>* __restrict__ sorted,
    const float4* __restrict__ sorted_v, const int* __restrict__ cube_id, const int* __restrict__ offs,
    const int gs, const int n_cubes, const float cube_size, const float gabriel_coefficient,
    Pt* __restrict__ d_dX, const bool has_gen, float* __restrict__ workspace, const long stride)
{
    float* x = workspace + GABRIEL_DENSE_ARRAYS * stride * blockIdx.x;
    for (int t = blockIdx.x; t < n_dense[0]; t += gridDim.x)
        gabriel_force_dense_cell<Pt, pw_int, pw_friction>(threadIdx.x, dense[t], 0, sorted, sorted_v, cube_id, offs, gs,
            n_cubes, cube_size, gabriel_coefficient, d_dX, has_gen, x, stride);
}

// fix = what is subtracted from dX.xyz: 0 = mean (already in d_mean), 1 = the
// fixed point's value, 2 = the point's x, y and the mean's z (set_fixed_xy,
// solvers.cuh:243-249).
template<typename Pt>
__global__ void make_fix(int mode, const float* __restrict__ d_mean,
    const Pt* __restrict__ d_point, float* __restrict__ d_fix)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (mode == 1) {
        d_fix[0] = d_point->x;
        d_fix[1] = d_point->y;
        d_fix[2] = d_point->z;
    } else {
        d_fix[0] = d_point->x;
        d_fix[1] = d_point->y;
        d_fix[2] = d_mean[2];
    }
}

// A fixed velocity that was computed in registers, `sum * float(1. / n)`, as the ROUNDED binary32 value that
// ya_reduce_mean would have left in memory.  The fast-arithmetic tier (YA_ARITH_FAST, -ffp-contract=fast, which
// disregards `#pragma clang fp contract(off)`; __fmul_rn is a plain `*` in HIP) is otherwise free to fuse the product
// into the update kernels' `dX - fix`, and did so in one instantiation (one use: v_fma_f32 d, -inv, sum, dX) and not
// in another (the four tiles of heun_step_sorted<Pt, true, 4> use it four times: v_mul_f32, v_sub_f32):
// take_step(dt, k) and k calls of take_step(dt, 1) then differed by one rounding of the centre-of-mass velocity per
// stage (tests/test_fast_tier_carry_gpu.py).  The empty statement makes the three values opaque to the optimiser
// where they are, in vector registers, and emits no instruction.  Without contraction there is nothing to fuse, and
// the exact tier is compiled without the statement: its instructions and their order stay what they were.
__device__ __forceinline__ void round_fix(float3& fix)
{
#ifdef YA_ARITH_FAST
    asm volatile("" : "+v"(fix.x), "+v"(fix.y), "+v"(fix.z));
#endif
}
// The fixed velocity from a z-slab stage's ALL-REDUCED totals (ya_slab_pack on every rank, summed):
// {sum[n_floats], count in two pieces, two votes, the fixed point's right-hand side}.
// fix_mode 0 (set_fixed()): fix = sum * float(1. / n), the reference's Pt / n arithmetic
// (dtypes.cuh:202-217; n through binary32 as there); 1 (set_fixed(i)): the fixed point's value,
// which only its owner put into the sum; 2 (set_fixed_xy(i), first stage): its x and y, the mean's z
// (solvers.cuh:241-253).
__device__ __forceinline__ float3 fix_from_total(const float* __restrict__ total, const int n_floats, const int fix_mode = 0)
{
    const double n = (double)total[n_floats] + 4096. * (double)total[n_floats + 1];
    const float inv = (float)(1. / (double)(float)n);
    float3 mean{total[0] * inv, total[1] * inv, total[2] * inv};
    round_fix(mean);
    if (fix_mode == 0) return mean;
    const float* point = total + n_floats + 4;
    return float3{point[0], point[1], fix_mode == 1 ? point[2] : mean.z};
}
// The drift guard of a z-slab weighs a cell's movement by where it was when the mirrored cells were
// chosen: fully within `width` = halo + limit of a face of the slab (those cells are mirrored, or
// next in line), half elsewhere -- a cell further away has to cover `limit` more before it can
// matter, so the guard's bound `limit` on the weighted maximum allows it 2 limit
// (include/slab_logic.inc, guard_between_stages).
struct Guard_band {
    float lo_face = -INFINITY, hi_face = INFINITY, width = 0.f;
    __host__ __device__ float weight(const float z) const
    {
        return fabsf(z - lo_face) <= width || fabsf(z - hi_face) <= width ? 1.f : 0.5f;
    }
};
// The largest v of the workgroup (v >= 0, or NaN: counted as +inf) folded into one of
// GUARD_SLOTS slots of `partial` by a non-returning atomic max (non-negative binary32 values order
// like their bit patterns); every thread of an UPDATE_BLOCK-wide workgroup must call it.  The slots
// are read, and zeroed again, by the reduction that follows (ya_slab_pack).  For the drift guard of
// a z-slab: thousands of workgroups, a few dozen atomics per slot, one short list to fold.
constexpr int GUARD_SLOTS = 256;
__device__ __forceinline__ void block_max_to(float v, float* __restrict__ partial)
{
    __shared__ float sh_max[UPDATE_BLOCK / 64];
    v = v == v ? v : INFINITY;
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < UPDATE_BLOCK / 64; w++) v = fmaxf(v, sh_max[w]);
        if (v > 0.f) atomicMax(reinterpret_cast<unsigned*>(partial) + (blockIdx.x % GUARD_SLOTS), __float_as_uint(v));
    }
}

// The mean of a stage's right-hand sides folded by the update kernel itself from the reduction's partial sums:
// ya_reduce_mean's second launch (4-5 us, four times per step at any system size) for a few hundred additions.
// Every workgroup repeats that fold from the partials (<= 1024 x 3 floats, L2 hits): the same additions in the
// same tree (lane t takes partials t, t + 256, ...; lanes folded by halving), the same `sum * float(1. / n)`
// (dtypes.cuh:202-217), hence the same bits as ya_reduce_mean leaves in d_mean -- only x, y, z, all the
// update kernels subtract (solvers.cuh:113-144).
template<int NF>
__device__ __forceinline__ float3 fixed_velocity_from_partials(const float* __restrict__ partials, const int n_partials,
    const int n)
{
    __shared__ float sh[3 * UPDATE_BLOCK];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int p = threadIdx.x; p < n_partials; p += UPDATE_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] = acc[k] + partials[(size_t)p * NF + k];
    }
    fold256<3>(acc, sh);
    const float inv = (float)(1. / (double)(float)n);  // Pt / n == Pt * float(1. / float(n))
    float3 mean{sh[0] * inv, sh[UPDATE_BLOCK] * inv, sh[2 * UPDATE_BLOCK] * inv};
    round_fix(mean);
    return mean;
}

// Where an update kernel takes a stage's fixed velocity from (solvers.cuh:241-253,265-272).  A template
// parameter: each kernel instance holds the code of its own source only.
//   memory    src[0..2], left by ya_reduce_mean (+ make_fix)
//   partials  src = ya_reduce_partials' `arg` partial sums, folded here (fixed_velocity_from_partials)
//   totals    src = a z-slab stage's all-reduced totals, arg = fix_mode (fix_from_total)
enum class Fix_src { memory, partials, totals };
struct Fix_args {
    const float* src = nullptr;
    int arg = 0;
    float* out = nullptr;  // predictor, may be NULL: its thread 0 leaves the velocity here for the corrector
};
// What the update kernels read and write of a computer that keeps the cells cube-sorted (Computer::carries; all null
// for one that does not).  The last four exist once Grid_computer::carry_ready has said so.
template<typename Pt>
struct Sorted_buffers {
    Entry<Pt>* cells = nullptr;          // the cube-sorted copy stage 1 kept (stage_update moves it)
    const Pt* rhs = nullptr;             // ... and its right-hand side in that order
    Entry<Pt>* carried = nullptr;        // a carried step: the predictor's output, then the corrector's
    float4* carried_v = nullptr;         // the corrector's {old_v, 0}
    const Pt* carried_rhs = nullptr;     // stage 2's right-hand sides in stage 2's sorted order
    const int* carried_slots = nullptr;  // stage-1 slot -> stage-2 slot
};
// Every thread of the workgroup calls it, before any early return: the partials fold has barriers.  What it
// returns is rounded (a value from memory is; a mean computed here goes through round_fix), so every update kernel
// subtracts the same bits whatever the contraction mode and however often it uses them.
template<Fix_src S, typename Pt>
__device__ __forceinline__ float3 resolve_fix(const Fix_args& f, const int n)
{
    if constexpr (S == Fix_src::memory)
        return float3{f.src[0], f.src[1], f.src[2]};
    else if constexpr (S == Fix_src::partials)
        return fixed_velocity_from_partials<N_floats<Pt>::value>(f.src, f.arg, n);
    else
        return fix_from_total(f.src, N_floats<Pt>::value, f.arg);
}
template<typename Pt>
__device__ __forceinline__ Pt minus_fix(Pt dX, const float3 fix)
{
    dX.x -= fix.x;
    dX.y -= fix.y;
    dX.z -= fix.z;
    return dX;
}
// The corrector's arithmetic for one cell, X += ((dX - fix) + (dX1 - fix1)) / 2 dt (solvers.cuh:127-144), from the
// two stages' raw right-hand sides; returns the cell's new old_v.  Every corrector kernel goes through here.
template<typename Pt>
__device__ __forceinline__ float3 heun_update(Pt& X, const Pt dX_raw, const Pt dX1_raw, const float3 fix,
    const float3 fix1, const float dt)
{
    const Pt dX = minus_fix(dX_raw, fix);
    const Pt dX1 = minus_fix(dX1_raw, fix1);
    X += (dX + dX1) * 0.5 * dt;
    return float3{(dX.x + dX1.x) * 0.5f, (dX.y + dX1.y) * 0.5f, (dX.z + dX1.z) * 0.5f};
}
// Row i of the corrector and old_v, fix = d_fix[0..2] as the predictor left it; returns the new X.  zero_dX: the
// row of d_dX, dead after this, is left zeroed for the next step's generic forces.
template<typename Pt>
__device__ __forceinline__ Pt heun_row(const int i, const float dt, const float* __restrict__ d_fix, const float3 fix1,
    Pt* __restrict__ d_dX, const Pt* __restrict__ d_dX1, Pt* __restrict__ d_X, float3* __restrict__ d_old_v,
    const bool zero_dX)
{
    const Pt dX_raw = d_dX[i];
    if (zero_dX) d_dX[i] = ya::zero<Pt>();  // (straight after the load: no address kept live)
    Pt X = d_X[i];
    d_old_v[i] = heun_update(X, dX_raw, d_dX1[i], float3{d_fix[0], d_fix[1], d_fix[2]}, fix1, dt);
    d_X[i] = X;
    return X;
}
}  // namespace ya


// 2nd order solver for the equation v = F + <v(t - dt)> for x, y, and z, where
// <v> is the mean velocity of the neighbours weighted by the friction
// coefficients; other variables in Pt follow dw/dt = F_w (solvers.cuh:109-144).
// The right-hand sides stay raw: the corrector subtracts both stages' fixed velocities.
//
// The predictor X1 = X0 + (dX - fix) dt (solvers.cuh:113-125) on every copy of the cells that is given, in one
// launch.  All pointers but d_dX may be NULL:
//   d_X0 -> d_X1  the cells in id order (what the generic forces are handed, and stage 2's input without a
//                 sorted copy)
//   d_sorted      the cube-sorted copy of Grid_solver, moved in place (or, d_sorted_out given, written there
//                 and left as it is: Heun_solver::take_steps), from which stage 2's grid build starts:
//                 a cell's right-hand side is d_dX_sorted[slot], or (totals source) d_dX[id] for a z-slab's
//                 mirrored cell (id >= n_active), which arrived by message in id order; the copy holds X[id] bit
//                 for bit, so both give the bits of d_X1[id]
//   d_zero        the next stage's right-hand side array, whose row i is dead by now: left zeroed for the
//                 generic forces that will add to it (a memset launch less)
//   pred_partial  (totals source) the largest |z moved| weighted by band, the drift guard of a z-slab
//                 (ya::block_max_to)
//   BIN           (a carried step, d_sorted given): the lane also bins the entry it stores, slot i, into the grid
//                 `bin` names (ya::bin_entry), so that the rebuild from these entries needs no k_bin launch
//                 (ya_grid_rebuild_sorted_binned); an instance without BIN holds none of that code
//   TILES         (a carried step) the workgroup takes TILES x UPDATE_BLOCK consecutive slots, thread t the slots
//                 base + UPDATE_BLOCK j + t, one round after the other: the fold of the partial sums, which every
//                 workgroup repeats, then runs in 1 / TILES as many of them.  Launch ceil(n / (TILES UPDATE_BLOCK)).
template<typename Pt, ya::Fix_src S, bool BIN = false, int TILES = 1>
__global__ __launch_bounds__(ya::UPDATE_BLOCK) void euler_step(const int n, const float dt, const ya::Fix_args fix_args,
    const Pt* __restrict__ d_dX, const Pt* __restrict__ d_X0, Pt* __restrict__ d_X1, const Pt* __restrict__ d_dX_sorted,
    ya::Entry<Pt>* __restrict__ d_sorted, const int n_active, Pt* __restrict__ d_zero, float* __restrict__ pred_partial,
    const ya::Guard_band band, ya::Entry<Pt>* __restrict__ d_sorted_out = nullptr, const ya::Grid_bin bin = {})
{
    static_assert(TILES == 1 || S == ya::Fix_src::partials, "block_max_to is called once per workgroup");
    const float3 fix = ya::resolve_fix<S, Pt>(fix_args, n);
#pragma unroll
    for (int tile = 0; tile < TILES; tile++) {
        const int i = (blockIdx.x * TILES + tile) * ya::UPDATE_BLOCK + threadIdx.x;
        if (i == 0 && fix_args.out) {
            fix_args.out[0] = fix.x;
            fix_args.out[1] = fix.y;
            fix_args.out[2] = fix.z;
        }
        float moved = 0.f;
        [[maybe_unused]] float3 at{0.f, 0.f, 0.f};  // BIN: where the entry of slot i is now
        if (i < n) {
            if (d_X1) {
                const Pt X0 = d_X0[i];
                const Pt X1 = X0 + ya::minus_fix(d_dX[i], fix) * dt;
                d_X1[i] = X1;
                moved = fabsf(X1.z - X0.z) * band.weight(X0.z);
            }
            if (d_sorted) {
                ya::Entry<Pt> e = d_sorted[i];
                Pt dX = d_dX_sorted[i];
                if constexpr (S == ya::Fix_src::totals)
                    if (e.id >= n_active) dX = d_dX[e.id];
                const float z0 = e.X.z;
                e.X = e.X + ya::minus_fix(dX, fix) * dt;
                (d_sorted_out ? d_sorted_out : d_sorted)[i] = e;
                moved = fabsf(e.X.z - z0) * band.weight(z0);
                if constexpr (BIN) at = float3{e.X.x, e.X.y, e.X.z};
            }
            if (d_zero) d_zero[i] = ya::zero<Pt>();
        }
        if constexpr (S == ya::Fix_src::totals)
            if (pred_partial) ya::block_max_to(moved, pred_partial);
        if constexpr (BIN) ya::bin_entry(bin, i < n, i, at.x, at.y, at.z);  // (every lane: shuffles, a ballot)
    }
}

// The corrector X += ((dX - fix) + (dX1 - fix1)) / 2 dt and old_v (solvers.cuh:127-144): fix is the first stage's
// velocity as the predictor left it (d_fix), fix1 comes from S.  (zero_dX: row i of d_dX, dead after this, is left
// zeroed for the next step's generic forces.  Totals source: z_selected / moved_partial, may be NULL: the largest
// |z - z when the mirrored cells were chosen| weighted by band, the drift guard; votes_out, may be NULL (host memory
// the device can write): the all-reduced votes of this stage, totals[n_floats + 2 .. + 3].)
template<typename Pt, ya::Fix_src S>
__global__ __launch_bounds__(ya::UPDATE_BLOCK) void heun_step(const int n, const float dt, const float* __restrict__ d_fix,
    const ya::Fix_args fix1_args, Pt* __restrict__ d_dX, const Pt* __restrict__ d_dX1, Pt* __restrict__ d_X,
    float3* __restrict__ d_old_v, const bool zero_dX, const float* __restrict__ z_selected,
    float* __restrict__ moved_partial, const ya::Guard_band band, float* __restrict__ votes_out)
{
    const float3 fix1 = ya::resolve_fix<S, Pt>(fix1_args, n);
    const int i = blockIdx.x * ya::UPDATE_BLOCK + threadIdx.x;
    float moved = 0.f;
    if (i < n) {
        const Pt X = ya::heun_row(i, dt, d_fix, fix1, d_dX, d_dX1, d_X, d_old_v, zero_dX);
        if (z_selected) moved = fabsf(X.z - z_selected[i]) * band.weight(z_selected[i]);
    }
    if constexpr (S == ya::Fix_src::totals) {
        if (votes_out && i == 0) {
            votes_out[0] = fix1_args.src[ya::N_floats<Pt>::value + 2];
            votes_out[1] = fix1_args.src[ya::N_floats<Pt>::value + 3];
        }
        if (moved_partial) ya::block_max_to(moved, moved_partial);
    }
}

// The corrector of a carried step (Heun_solver::take_steps), one thread per slot of the step's FIRST build: the
// cell and its id from d_sorted[s], still at the step's start; stage 1's right-hand side in that order; stage 2's
// at d_slot2[s], where the second build put the cell (near s: cells move little).  Same operands and statements
// as heun_step (ya::heun_update).  Leaves {X, id} and {old_v, 0} in slot s of d_out / d_out_v, from which the
// next step's first build starts, and -- the call's last step: d_X, d_old_v given -- the id-ordered arrays.
// BIN: the lane also bins the entry it leaves in slot s for that next build (ya::bin_entry, as euler_step's);
// whole wavefronts reach the binning, so no lane leaves early.  TILES: as euler_step's.
template<typename Pt, bool BIN = false, int TILES = 1>
__global__ __launch_bounds__(ya::UPDATE_BLOCK) void heun_step_sorted(const int n, const float dt,
    const float* __restrict__ d_fix, const ya::Fix_args fix1_args, const ya::Entry<Pt>* __restrict__ d_sorted,
    const Pt* __restrict__ d_dX_sorted, const int* __restrict__ d_slot2, const Pt* __restrict__ d_dX1_sorted,
    ya::Entry<Pt>* __restrict__ d_out, float4* __restrict__ d_out_v, Pt* __restrict__ d_X, float3* __restrict__ d_old_v,
    const ya::Grid_bin bin = {})
{
    const float3 fix1 = ya::resolve_fix<ya::Fix_src::partials, Pt>(fix1_args, n);
    const float3 fix{d_fix[0], d_fix[1], d_fix[2]};
#pragma unroll
    for (int tile = 0; tile < TILES; tile++) {
        const int s = (blockIdx.x * TILES + tile) * ya::UPDATE_BLOCK + threadIdx.x;
        [[maybe_unused]] float3 at{0.f, 0.f, 0.f};  // BIN: where the entry of slot s is now
        if (s < n) {
            ya::Entry<Pt> e = d_sorted[s];
            const float3 v = ya::heun_update(e.X, d_dX_sorted[s], d_dX1_sorted[d_slot2[s]], fix, fix1, dt);
            d_out[s] = e;
            d_out_v[s] = make_float4(v.x, v.y, v.z, 0.f);
            if (d_X) {
                d_X[e.id] = e.X;
                d_old_v[e.id] = v;
            }
            if constexpr (BIN) at = float3{e.X.x, e.X.y, e.X.z};
        }
        if constexpr (BIN) ya::bin_entry(bin, s < n, s, at.x, at.y, at.z);
    }
}


// ---- renumbering (opt-in, not in the reference) ---------------------------------------------------
// Solution::renumber(properties ...) gives the cells new ids in cube order: the cell in slot s of
// a fresh grid build becomes cell s.  The reference's contract is that ids never change -- models
// index their own per-cell arrays by id (d_type[i], examples/passive_growth.cu:48-51) and append
// daughters at d_X[n] -- so a model that has grown by division holds its cells in birth order,
// spatially random, and every access of a pairwise functor to such an array (four per interacting
// pair in passive_growth's relu_w_epithelium) is 64 different cache lines per wavefront
// instruction: BASELINE configuration 4 moved 6.7 GB between L2 and the fabric per force launch
// where 70 MB are needed, 78 % of its wave cycles waiting (profiles/r03_pmc_cfg4_*).  Only the
// model knows all arrays that are indexed by cell id, so only the model can ask for a
// renumbering, handing over every such array:
//
//     if (step % 10 == 0) cells.renumber(type, n_mes_nbs, n_epi_nbs);   // Property<...>&, Links&, or T* d_array
//
// Afterwards cell s is what cell order[s] was (d_X, d_old_v and the arrays handed over are
// permuted alike, link endpoints are renamed), consecutive ids are neighbours in space, and so
// are the daughters a proliferation kernel appends later in the order of their mothers.  Host
// mirrors (h_X, h_prop) are stale until the next copy_to_host.  Results: every per-cell sum is
// still accumulated cube by cube in ascending id, and the stable sort keeps the order of ids
// inside a cube across the renumbering, so forces change only through cells that later move
// between cubes (rounding of reordered sums); a model that draws random numbers by cell id draws
// others.  The CPU oracle offers the same call (oracle/yalla_host.hpp) and both backends stay in
// lock-step through it (tests/test_growth.py).
namespace ya {
template<typename T>
__global__ __launch_bounds__(UPDATE_BLOCK) void permute_rows(const int n, const int* __restrict__ order,
    const T* __restrict__ src, T* __restrict__ dst)
{
    const int s = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    if (s < n) dst[s] = src[order[s]];
}
__global__ __launch_bounds__(UPDATE_BLOCK) void invert_order(const int n, const int* __restrict__ order,
    int* __restrict__ new_id)
{
    const int s = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    if (s < n) new_id[order[s]] = s;
}
// link endpoints (two ints per link: links.cuh Link{a, b}) renamed through new_id; ids >= n (none in a
// consistent model) are left alone
__global__ __launch_bounds__(UPDATE_BLOCK) void rename_ids(const int n_ids, const int* __restrict__ d_n_links,
    const int n_cells, const int* __restrict__ new_id, int* __restrict__ ids)
{
    const int k = blockIdx.x * UPDATE_BLOCK + threadIdx.x;
    if (k >= n_ids || k >= 2 * *d_n_links) return;
    const int i = ids[k];
    if (i >= 0 && i < n_cells) ids[k] = new_id[i];
}
}  // namespace ya


// Solution<Pt, Solver> combines a method, Solver, with a point type, Pt: host
// mirror of the variables plus access to the device arrays (solvers.cuh:56-106).
template<typename Pt, template<typename> class Solver>
class Solution : public Solver<Pt> {
public:
    Pt* h_X;                                      // Current variables on host
    Pt* const d_X = Solver<Pt>::d_X;              // Variables on device (GPU)
    float3* const d_old_v = Solver<Pt>::d_old_v;  // Velocities from previous step
    int* const h_n = (int*)malloc(sizeof(int));   // Number of points
    int* const d_n = Solver<Pt>::d_n;
    const int n_max;
    template<typename... Args>
    Solution(int n_max, Args... args) : Solver<Pt>{n_max, args...}, n_max{n_max}
    {
        *h_n = n_max;
        // page-locked if the runtime grants it: a frame's copy_to_host moves all n_max points
        // (26 MB at config 4); zeroed like calloc'ed memory
        const size_t bytes = (size_t)n_max * sizeof(Pt);
        h_X_locked = n_max > 0 && ya_host_alloc((void**)&h_X, bytes) == 0;
        if (h_X_locked)
            memset((void*)h_X, 0, bytes);
        else
            h_X = (Pt*)calloc(n_max, sizeof(Pt));
    }
    ~Solution()
    {
        if (h_X_locked)
            (void)ya_host_free(h_X);
        else
            free(h_X);
        free(h_n);
    }
    Solution(const Solution&) = delete;

private:
    bool h_X_locked = false;
    // a z-slab decomposition (Slab_grid_solver, slab.on) steps through its own take_step
    template<typename S>
    static auto decomposed(const S& solver, int) -> decltype((bool)solver.slab.on)
    {
        return solver.slab.on;
    }
    template<typename S>
    static bool decomposed(const S&, long)
    {
        return false;
    }

public:
    void copy_to_device()
    {
        assert(*h_n <= n_max);
        YA_CHECK(ya_memcpy_h2d(d_X, h_X, (size_t)n_max * sizeof(Pt)));
        YA_CHECK(ya_memcpy_h2d(d_n, h_n, sizeof(int)));
    }
    void copy_to_host()
    {
        YA_CHECK(ya_memcpy_d2h(h_X, d_X, (size_t)n_max * sizeof(Pt)));
        YA_CHECK(ya_memcpy_d2h(h_n, d_n, sizeof(int)));
        assert(*h_n <= n_max);
        Solver<Pt>::check_status();
    }
    int get_d_n() { return Solver<Pt>::get_d_n(); }
    template<Pairwise_interaction<Pt> pw_int>
    void take_step(float dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        return Solver<Pt>::template take_step<pw_int, friction_w_neighbour<Pt>>(
            dt, gen_forces);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_step(float dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        return Solver<Pt>::template take_step<pw_int, pw_friction>(dt, gen_forces);
    }
    // k steps in one call (not in the reference): bit for bit what k calls of take_step leave, with the
    // same generic force in each.  Between the steps of one call nothing outside the engine sees or
    // changes the cells, which lets Grid_solver keep them in cube order from step to step
    // (Heun_solver::take_steps).
    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(float dt, int k, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, k, gen_forces);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(float dt, int k, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        if (!decomposed(*this, 0)) return Solver<Pt>::template take_steps<pw_int, pw_friction>(dt, k, gen_forces);
        for (int s = 0; s < k; s++) Solver<Pt>::template take_step<pw_int, pw_friction>(dt, gen_forces);
    }
    // The former two-argument generic force `(const Pt* d_X, Pt* d_dX)`, which the
    // reference's own tests still use (tests/test_solvers.cu:141, test_links.cu:19).
    template<Pairwise_interaction<Pt> pw_int, typename Gen2,
        typename = decltype(std::declval<Gen2&>()((const Pt*)nullptr, (Pt*)nullptr))>
    void take_step(float dt, Gen2 gen_forces)
    {
        take_step<pw_int>(dt, Generic_forces<Pt>{[gen_forces](const int, const Pt* d_X,
                                                     Pt* d_dX) mutable { gen_forces(d_X, d_dX); }});
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Gen2,
        typename = decltype(std::declval<Gen2&>()((const Pt*)nullptr, (Pt*)nullptr))>
    void take_step(float dt, Gen2 gen_forces)
    {
        take_step<pw_int, pw_friction>(dt,
            Generic_forces<Pt>{[gen_forces](const int, const Pt* d_X, Pt* d_dX) mutable {
                gen_forces(d_X, d_dX);
            }});
    }
};


// The three-parameter spelling `Solution<Pt, n_max, Solver>` of older ya||a model files (and of this
// build's north_star): the capacity as a template argument, objects default-constructed.  C++ cannot
// overload a class template on the KIND of its parameters, so beside the reference's two-parameter
// `Solution<Pt, Solver>{n_max, ...}` (every example at the surveyed commit) it has a name of its own:
//     Solution_n<float3, 800, Tile_solver> bodies;            // = Solution<float3, Tile_solver>{800}
//     Solution_n<float3, 100000, Grid_solver> cells{64, 1.f}; // solver arguments follow as usual
template<typename Pt, int N_MAX, template<typename> class Solver>
class Solution_n : public Solution<Pt, Solver> {
public:
    static constexpr int capacity = N_MAX;
    template<typename... Args>
    Solution_n(Args... args) : Solution<Pt, Solver>{N_MAX, args...}
    {}
};


// Two-stage Heun integrator (solvers.cuh:164-276).  Computer specifies how
// pairwise interactions are computed.
template<typename Pt, template<typename> class Computer>
class Heun_solver : public Computer<Pt> {
public:
    template<typename... Args>
    Heun_solver(int n_max, Args... args) : Computer<Pt>{n_max, args...}, n_max{n_max}
    {
        const size_t pts = (size_t)n_max * sizeof(Pt);
        YA_CHECK(ya_malloc((void**)&d_X, pts));
        YA_CHECK(ya_malloc((void**)&d_dX, pts));
        YA_CHECK(ya_malloc((void**)&d_X1, pts));
        YA_CHECK(ya_malloc((void**)&d_dX1, pts));
        YA_CHECK(ya_malloc((void**)&d_old_v, (size_t)n_max * sizeof(float3)));
        YA_CHECK(ya_memset_async(d_old_v, 0, (size_t)n_max * sizeof(float3), nullptr));
        YA_CHECK(ya_malloc((void**)&d_n, sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_mean, 2 * sizeof(Pt)));
        YA_CHECK(ya_malloc((void**)&d_mean_first, 2 * sizeof(Pt)));
        YA_CHECK(ya_n_reader_create(&n_reader));
        YA_CHECK(ya_malloc((void**)&d_fix, 4 * sizeof(float)));
        YA_CHECK(ya_malloc((void**)&d_fix_first, 4 * sizeof(float)));
        YA_CHECK(ya_malloc((void**)&d_workspace, ya_reduce_workspace_bytes(n_floats)));
    }
    ~Heun_solver()
    {
        ya_free(d_X);
        ya_free(d_dX);
        ya_free(d_X1);
        ya_free(d_dX1);
        ya_free(d_old_v);
        ya_free(d_n);
        ya_free(d_mean);
        ya_free(d_mean_first);
        ya_n_reader_destroy(n_reader);
        ya_free(d_fix);
        ya_free(d_fix_first);
        ya_free(d_workspace);
        if (renumber_scratch) ya_free(renumber_scratch);
        drop_graph();
        if (capture_stream) (void)hipStreamDestroy(capture_stream);
    }
    Heun_solver(const Heun_solver&) = delete;
    void set_fixed() { fix_com = true; }
    void set_fixed(int point_id)
    {
        fix_com = false;
        fix_point = point_id;
    }
    void set_fixed_xy(int point_id)
    {
        fix_com = false;
        fix_com_z = true;
        fix_point = point_id;
    }
    // Opt-in, not in the reference: new cell ids in cube order (see "renumbering" above).  Hand
    // over EVERY array the model indexes by cell id: Property<T>& (anything with a d_prop member),
    // Links& (anything with d_link / d_n: the endpoints are renamed), or a plain device pointer
    // T* of >= n elements.  No-op for solvers without a grid (Tile_solver).
    template<typename... Arrays>
    void renumber(Arrays&... arrays)
    {
        const int n = get_d_n();
        if (n <= 0) return;
        if constexpr (has_grid) {
            const int* order = Computer<Pt>::cube_order(n, d_X);  // order[s] = the id of the cell in slot s
            permute_array(order, n, d_X);
            permute_array(order, n, d_old_v);
            int* new_id = nullptr;
            const int unused[] = {0, (renumber_one(order, n, arrays, new_id), 0)...};
            (void)unused;
            if (new_id) ya_free(new_id);
            rhs_zeroed[0] = rhs_zeroed[1] = 0;  // (nothing here writes d_dX / d_dX1; no promise is carried over a renumbering)
            Computer<Pt>::ids_changed();
            // a graph captured NOW would bake the forgotten visit order (n_prev = 0) into its first build:
            // capture again one step later, when the grid remembers an order again
            drop_graph();
            last_key = Step_key{};
        }
    }

    // ... or ONE line after the model has made its arrays, instead of a call in its loop (round 5):
    //     cells.keep_in_cube_order(10, type, n_mes_nbs, n_epi_nbs, links, d_state);
    // -- every `every`-th take_step (the next one first) begins with renumber(arrays...).  The arrays are
    // taken by reference: they must outlive the solver's steps, as they must in a loop that calls
    // renumber itself.  every <= 0 switches it off again.  Cells a model kernel appended since the last
    // renumbering (proliferation) are put in their places by the next one.
    template<typename... Arrays>
    void keep_in_cube_order(const int every, Arrays&... arrays)
    {
        keep_order_every = every;
        keep_order_wait = 0;
        if (every > 0)
            keep_order = [this, &arrays...]() { this->renumber(arrays...); };
        else
            keep_order = nullptr;
    }

    // Replaying the step as one hipGraph (Grid_solver without generic forces), opt-in:
    // 1 = whenever possible, -1 = for systems below YA_GRAPH_MAX_CELLS cells, 0 (default) =
    // never.  The graph is captured the second time in a row the same step is asked for and
    // replayed while that stays so.  "The same step" is everything a captured launch bakes in
    // (Step_key): functors, n, dt, fixed mode and point, fold_in_update, cube size, and the
    // computer's own settings (Grid_computer::step_variant: force_variant, sum_order, coop_lanes,
    // stage_v_max, force_tail_tiles, d_global_id, the tail exchange areas).  These are public
    // members a model may assign at any time, so they are compared at every step, not watched
    // by setters.  The step after ANY change is a plain one (it may allocate, and it leaves the
    // grid's remembered visit order as a replay expects it); a graph whose key comes back is
    // replayed again from the step after that.  A changing n (proliferation) simply keeps the
    // plain launches.  Results are identical: the same kernels with the same arguments.
    // graph_launches counts the hipGraphLaunch calls.  Measured on MI355X it buys nothing when the
    // host queues launches from a C++ loop (a step of a 10^4-cell system is bound by the
    // ~18 dependent kernels' own latencies, 0.19 ms either way); it is for hosts that
    // cannot keep ~10^5 launches per second up.
    int graph_steps = 0;
    long graph_launches = 0;  // read-only: steps that ran as a hipGraphLaunch (tests: replay really happened)
    // take_steps: false = always the loop of take_step (A/B, tests; same results)
    bool carry_sorted = true;
    long carried_steps = 0;  // read-only: steps whose first build started from the step before's cube-sorted cells
    // carried steps: the update kernels bin the entries they store (euler_step / heun_step_sorted<BIN>), and the
    // rebuild behind them runs without k_bin; false = k_bin as before (A/B, tests; same results)
    bool bin_in_update = true;
    // ... and those rebuilds whose public point ids nobody can read skip storing them (YA_REBUILD_PRIVATE);
    // false = every rebuild stores them (A/B; same results).  Only with bin_in_update.
    bool trim_carried_stores = true;
    // ... and their workgroups take four tiles of UPDATE_BLOCK slots each (euler_step / heun_step_sorted<TILES>);
    // false = one (A/B; same results).  Only with bin_in_update.
    bool four_tile_updates = true;
    long fused_bin_rebuilds = 0;  // read-only: rebuilds that ran without k_bin, 2 k - 1 per carried call of k steps

protected:
#ifndef YA_GRAPH_MAX_CELLS
#define YA_GRAPH_MAX_CELLS 400000
#endif
    struct Step_key {
        const void* functors = nullptr;
        int n = -1;
        float dt = 0, cube_size = 0;
        typename Computer<Pt>::Step_variant variant{};
        int fix_mode = 0, fix_point = 0;
        bool fold = true;
        auto tied() const { return std::tie(functors, n, dt, cube_size, variant, fix_mode, fix_point, fold); }
        bool operator==(const Step_key& o) const { return tied() == o.tied(); }
    };
    Step_key graph_key, last_key;
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t capture_stream = nullptr;
    void drop_graph()
    {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        graph_exec = nullptr;
        graph_key = Step_key{};
    }
    static constexpr int n_floats = ya::N_floats<Pt>::value;
    // libyalla_hip.so's reductions, grid builds and packs are built per width, for 3 to 16 floats: a wider point would
    // end in hipErrorInvalidValue from them at the first step
    static_assert(n_floats >= 3 && n_floats <= 16, "yalla-hip: a point type has 3 to 16 floats (the 16-float limit of "
                                                   "libyalla_hip.so's per-width kernels)");
    Pt *d_X, *d_dX, *d_X1, *d_dX1;
    float3* d_old_v;
    int* d_n;
    float *d_mean, *d_fix, *d_mean_first, *d_fix_first, *d_workspace;
    ya_n_reader* n_reader = nullptr;
    int sorted_stage_cells = -1;  // cells in the sorted copy stage 1 kept: stage_update(1) moves it, stage 2 starts from it
    const float* stage1_fix = nullptr;  // where stage_update(1) left the first stage's fixed velocity for the corrector
    // rows of d_dX / d_dX1 an update kernel left zeroed (stage_update).  INVARIANT: every writer of those two arrays
    // goes through stage_rhs (which resets the promise) -- the arrays are protected members and no accessor hands
    // them out; a new path that writes them must reset rhs_zeroed as well.
    int rhs_zeroed[2] = {0, 0};
    std::function<void()> keep_order;  // keep_in_cube_order: renumber(the registered arrays)
    int keep_order_every = 0, keep_order_wait = 0;
    bool fix_com = true;
    bool fix_com_z = false;
    // set_fixed(): the update kernels fold the reductions' partial sums themselves
    // (ya::fixed_velocity_from_partials; false = ya_reduce_mean's second launch, A/B)
    bool fold_in_update = true;
    int fix_point = 0;
    const int n_max;
    int get_d_n()
    {
        int n;
        YA_CHECK(ya_get_n(d_n, &n));
        assert(n <= n_max);
        return n;
    }
    void check_status() { if constexpr (has_grid) Computer<Pt>::check_status(); }
    // A computer's traits.  has_grid: the code for a grid (renumbering, the status, the cube-sorted copy of the cells
    // kept between stages and steps, captured steps) is compiled for such computers only, so Tile_computer declares
    // none of the members it calls.  carries: whether a computer with a grid keeps that copy at all (Gabriel's: no).
    static constexpr bool has_grid = Computer<Pt>::has_grid;
    bool sorted_pipeline_on() const
    {
        if constexpr (has_grid) return Computer<Pt>::carries && Computer<Pt>::use_sorted_pipeline();
        return false;
    }
    // set_fixed() (the default) with fold_in_update: the update kernel folds the mean from the reduction's partial sums
    bool update_folds_mean() const { return fix_com and !fix_com_z and fold_in_update; }
    // renumber(): array[s] = array[order[s]] for s < n, through a scratch buffer that is kept
    void* renumber_scratch = nullptr;
    size_t renumber_scratch_bytes = 0;
    template<typename T>
    void permute_array(const int* order, const int n, T* d_array)
    {
        const size_t bytes = (size_t)n * sizeof(T);
        if (renumber_scratch_bytes < bytes) {
            if (renumber_scratch) ya_free(renumber_scratch);
            renumber_scratch_bytes = 0;
            YA_CHECK(ya_malloc(&renumber_scratch, (size_t)n_max * sizeof(T) > bytes ? (size_t)n_max * sizeof(T) : bytes));
            renumber_scratch_bytes = (size_t)n_max * sizeof(T) > bytes ? (size_t)n_max * sizeof(T) : bytes;
        }
        ya::permute_rows<T><<<(n + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK, ya::UPDATE_BLOCK>>>(
            n, order, d_array, (T*)renumber_scratch);
        YA_CHECK(ya_memcpy_d2d_async(d_array, renumber_scratch, bytes, nullptr));
    }
    template<typename T>
    void renumber_one(const int* order, const int n, T*& d_array, int*&)
    {
        permute_array(order, n, d_array);
    }
    template<typename A>
    auto renumber_one(const int* order, const int n, A& property, int*&) -> decltype((void)property.d_prop)
    {
        permute_array(order, n, property.d_prop);
    }
    template<typename L>
    auto renumber_one(const int* order, const int n, L& links, int*& new_id) -> decltype((void)links.d_link)
    {
        if (!new_id) {
            YA_CHECK(ya_malloc((void**)&new_id, (size_t)n * sizeof(int)));
            ya::invert_order<<<(n + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK, ya::UPDATE_BLOCK>>>(n, order, new_id);
        }
        const int n_ids = 2 * links.n_max;
        ya::rename_ids<<<(n_ids + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK, ya::UPDATE_BLOCK>>>(
            n_ids, links.d_n, n, new_id, reinterpret_cast<int*>(links.d_link));
    }

    // The velocity subtracted from dX.xyz for this stage, left in device memory (first: stage 1's, which the
    // corrector reads after the second stage's reduction).
    const float* fix_velocity(int n, Pt* d_rhs, bool mean, bool point_xy, bool first = false)
    {
        float* mean_out = first ? d_mean_first : d_mean;
        float* fix_out = first ? d_fix_first : d_fix;
        if (mean) {  // solvers.cuh:241-249 / :266-268
            YA_CHECK(ya_reduce_mean(d_rhs, n_floats, n, mean_out, d_workspace, this->stream));
            if (!point_xy) return mean_out;
            ya::make_fix<Pt><<<1, 1, 0, this->stream>>>(2, mean_out, d_rhs + fix_point, fix_out);
            return fix_out;
        }
        ya::make_fix<Pt><<<1, 1, 0, this->stream>>>(1, mean_out, d_rhs + fix_point, fix_out);  // :250-253
        return fix_out;
    }

    // The pieces of a stage -- forces, then the source of the fixed velocity, then the update (stage 1 works on
    // d_X -> d_dX, stage 2 on d_X1 -> d_dX1).  take_step composes them (heun_stages); a z-slab decomposition
    // calls them one by one with a ghost exchange and an all-reduce in between (n = own + ghost cells,
    // n_active = own cells).
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void stage_rhs(int stage, int n, int n_active, Generic_forces<Pt>& gen_forces)
    {
        Pt* d_in = stage == 1 ? d_X : d_X1;
        Pt* d_rhs = stage == 1 ? d_dX : d_dX1;
        const bool has_gen = !ya::is_no_gen_forces<Pt>(gen_forces);
        if (has_gen) {
            // (the update kernel before this stage may have left the rows zeroed already: stage_update)
            if (rhs_zeroed[stage - 1] < n) YA_CHECK(ya_memset_async(d_rhs, 0, (size_t)n * sizeof(Pt), nullptr));
            gen_forces(n, d_in, d_rhs);
        }
        rhs_zeroed[stage - 1] = 0;  // the force kernel writes it next
        if constexpr (has_grid)
            if (stage == 2 && sorted_stage_cells == n) {
                // the second stage starts from the sorted copy stage_update(1) moved, mirrored cells included (the
                // generic forces above were given d_X1, as the reference does)
                sorted_stage_cells = -1;
                Computer<Pt>::template pwints_from_sorted<pw_int, pw_friction>(n, d_dX1, n_active, has_gen);
                return;
            }
        const bool keep_sorted = stage == 1 && sorted_pipeline_on();
        Computer<Pt>::template pwints<pw_int, pw_friction>(n, d_in, d_old_v, d_rhs, has_gen, n_active, keep_sorted);
        sorted_stage_cells = keep_sorted ? n : -1;
    }
    // sum and mean of the stage's right-hand side over the first n points, left on
    // the device as {mean[n_floats], sum[n_floats]}
    const float* stage_sum(int stage, int n)
    {
        YA_CHECK(ya_reduce_mean(
            stage == 1 ? d_dX : d_dX1, n_floats, n, d_mean, d_workspace, nullptr));
        return d_mean;
    }
    // What the update kernels leave for a z-slab (totals source; each may be NULL): the drift guard's maxima,
    // ya::GUARD_SLOTS floats each (zeroed by the reduction that reads them), and the all-reduced votes
    // (see heun_step)
    struct Slab_outputs {
        float* pred_partial = nullptr;      // stage 1
        const float* z_selected = nullptr;  // stage 2
        float* moved_partial = nullptr;
        float* votes_out = nullptr;
        ya::Guard_band band;
    };
    using Fix = ya::Fix_src;
    // The update of a stage, one launch, with the fixed velocity from S.  The right-hand sides stay raw; stage 1
    // leaves its velocity for the corrector.  Stage 1 moves the sorted copy that stage_rhs kept, and writes d_X1
    // only where it is read: by the generic forces, or by stage 2 without a sorted copy.  With generic forces
    // the kernels leave the right-hand side array of the NEXT stage zeroed -- d_dX1 after the predictor, d_dX
    // after the corrector: both dead by then -- so that the memset in front of the generic forces
    // (solvers.cuh:232,258 `thrust::fill`) need not be launched (rhs_zeroed: rows known to be zero).
    template<ya::Fix_src S>
    void stage_update(int stage, int n, float dt, ya::Fix_args fix, bool has_gen, int n_active,
        const Slab_outputs& slab_out = Slab_outputs{})
    {
        const int blocks = (n + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK;
        if (stage == 1) {
            const bool in_sorted = sorted_stage_cells == n;
            fix.out = S == Fix::memory ? nullptr : d_mean_first;
            stage1_fix = S == Fix::memory ? fix.src : d_mean_first;
            ya::Sorted_buffers<Pt> sorted;  // (all null without a grid)
            if constexpr (has_grid) sorted = Computer<Pt>::sorted_buffers();
            euler_step<Pt, S><<<blocks, ya::UPDATE_BLOCK, 0, this->stream>>>(n, dt, fix, d_dX, d_X,
                has_gen || !in_sorted ? d_X1 : nullptr, sorted.rhs, in_sorted ? sorted.cells : nullptr, n_active,
                has_gen ? d_dX1 : nullptr, slab_out.pred_partial, slab_out.band);
            rhs_zeroed[1] = has_gen ? n : 0;
        } else {
            heun_step<Pt, S><<<blocks, ya::UPDATE_BLOCK, 0, this->stream>>>(n, dt, stage1_fix, fix, d_dX, d_dX1, d_X,
                d_old_v, has_gen, slab_out.z_selected, slab_out.moved_partial, slab_out.band, slab_out.votes_out);
            rhs_zeroed[0] = has_gen ? n : 0;
        }
    }
    // what a rank puts into a stage's all-reduce (ya_slab_pack): the sum over its first n points and
    // their count, its two votes (the drift guard brought up to date in the same kernel if
    // fold_guard), the fixed point's right-hand side if *d_fix_index is one of its cells
    struct Guard_inputs {
        float* moved_partial = nullptr;
        int n_moved = 0;
        float* pred_partial = nullptr;
        int n_pred = 0;
        float limit = 0.f, lag_steps = 0.f;
        float* state = nullptr;
    };
    void stage_sum_packed(int stage, int n, float* d_out, const Guard_inputs& guard = Guard_inputs{}, int fold_guard = 0,
        int with_votes = 0, int host_error = 0, const int* d_fix_index = nullptr)
    {
        YA_CHECK(ya_slab_pack(stage == 1 ? d_dX : d_dX1, n_floats, n, d_out, d_workspace, guard.moved_partial, guard.n_moved,
            guard.pred_partial, guard.n_pred, guard.limit, guard.lag_steps, guard.state, fold_guard, with_votes, host_error,
            d_fix_index, nullptr));
    }

    // One step of n cells: per stage the forces, the fixed velocity, the update.  Without generic forces on
    // Grid_solver (the headline path, and the step a graph captures) the predictor lives in the cube-sorted copy
    // of the cells, so the second grid build gathers nothing and d_X1 is never materialised.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void heun_stages(const int n, const float dt, Generic_forces<Pt>& gen_forces)
    {
        const bool has_gen = !ya::is_no_gen_forces<Pt>(gen_forces);
        for (int stage = 1; stage <= 2; stage++) {
            stage_rhs<pw_int, pw_friction>(stage, n, n, gen_forces);
            Pt* d_rhs = stage == 1 ? d_dX : d_dX1;
            if (update_folds_mean()) {
                // (ya::fixed_velocity_from_partials: a launch fewer per stage, the same bits)
                int n_partials = 0;
                YA_CHECK(ya_reduce_partials(d_rhs, n_floats, n, d_workspace, &n_partials, this->stream));
                stage_update<Fix::partials>(stage, n, dt, {d_workspace, n_partials}, has_gen, n);
            } else {
                // set_fixed_xy(i) holds x and y in the first stage only (solvers.cuh:241-253, 265-272)
                const bool xy = stage == 1 && fix_com_z;
                stage_update<Fix::memory>(stage, n, dt, {fix_velocity(n, d_rhs, fix_com or xy, xy, stage == 1)}, has_gen, n);
            }
        }
    }

    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    Step_key key_of(const int n, const float dt)
    {
        static const char functors_tag = 0;  // one per <pw_int, pw_friction>
        Step_key k{&functors_tag, n, dt};
        if constexpr (has_grid) {
            k.cube_size = this->cube_size;
            k.variant = Computer<Pt>::step_variant();
        }
        k.fix_mode = (fix_com ? 1 : 0) | (fix_com_z ? 2 : 0);
        k.fix_point = fix_point;
        k.fold = fold_in_update;
        return k;
    }
    // The number of cells of the step that begins; <= 0: there is none (a build begun is cancelled).
    // build_ahead: the reference reads n first (solvers.cuh:229) and so must we, model kernels change it between
    // steps; but the round trip is hidden behind the binning kernels of the first grid build, which read the count
    // on the device.  (Round 5: with generic forces too.  They need n on the host -- gen_forces(n, d_X, d_dX) --
    // but the first build reads d_X only and the generic forces write d_dX only, so the build's first three kernels
    // may run before them: the device works while the count travels, instead of standing idle between two steps.
    // Round 6: the count travels in the first binning kernel itself, ya_grid_build_sorted_begin_publish, not in a
    // 4-byte copy queued ahead of it: one 4 us kernel fewer in the stream per step.)
    int read_n(const bool build_ahead)
    {
        if constexpr (has_grid) {
            int n = build_ahead ? 0 : get_d_n();
            if (build_ahead) {
                Computer<Pt>::begin_build(d_X, d_n, n_max, n_reader);
                YA_CHECK(ya_n_read_end(n_reader, &n));
                assert(n <= n_max);
            }
            if (n <= 0) Computer<Pt>::cancel_build();
            return n;
        }
        return get_d_n();
    }
    // The step of n cells as one hipGraphLaunch, a replay or a capture and its first launch; false = nothing was done
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    bool graph_step(const int n, const float dt, Generic_forces<Pt>& gen_forces)
    {
        const Step_key key = key_of<pw_int, pw_friction>(n, dt);
        // Replay only what the step before was too (key == last_key: every plain step leaves its key
        // there).  The graph also bakes in what the grid remembered when it was captured -- the visit
        // order of a build of these n cells (n_prev, d_prev_pid) -- and that holds only straight after
        // such a step: a graph whose key comes back after other steps (n down and up again) waits one
        // plain step.
        if (graph_exec && key == graph_key && key == last_key) {
            YA_CHECK((int)hipGraphLaunch(graph_exec, nullptr));
            graph_launches++;
            return true;
        }
        // NOTHING between hipStreamBeginCapture and hipStreamEndCapture may synchronise, allocate, free or
        // use the null stream (ya_device_synchronize, ya_malloc / ya_free, hipMemcpy, a memset or launch
        // without this->stream): the runtime fails such a call and YA_CHECK ends the process.  The step
        // before ran the same launches plainly, so everything lazily sized exists (the grid's stash, the
        // tail exchange area); a computer that would still have to allocate says so (ready_to_capture)
        // and the step stays a plain one.  The same step as last time is captured (thread-local mode: other
        // host threads of the model, e.g. one writing output, may keep using HIP).
        if (!(key == last_key && (graph_steps > 0 || n < YA_GRAPH_MAX_CELLS) &&
                Computer<Pt>::template ready_to_capture<pw_int, pw_friction>(n)))
            return false;
        drop_graph();
        if (!capture_stream) YA_CHECK((int)hipStreamCreateWithFlags(&capture_stream, hipStreamNonBlocking));
        YA_CHECK((int)hipStreamBeginCapture(capture_stream, hipStreamCaptureModeThreadLocal));
        this->stream = capture_stream;
        heun_stages<pw_int, pw_friction>(n, dt, gen_forces);
        this->stream = nullptr;
        hipGraph_t graph = nullptr;
        YA_CHECK((int)hipStreamEndCapture(capture_stream, &graph));
        YA_CHECK((int)hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
        YA_CHECK((int)hipGraphDestroy(graph));
        graph_key = key;
        YA_CHECK((int)hipGraphLaunch(graph_exec, nullptr));
        graph_launches++;
        return true;
    }

    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_step(float dt, Generic_forces<Pt> gen_forces)
    {
        if (keep_order && keep_order_wait-- <= 0) {  // keep_in_cube_order
            keep_order();
            keep_order_wait = keep_order_every - 1;
        }
        const bool sorted_path = sorted_pipeline_on() && ya::is_no_gen_forces<Pt>(gen_forces);
        // a small system whose steps may run as a graph reads n first, then replays / captures / launches
        const bool graph = sorted_path && graph_steps != 0 && last_key.n > 0 && !Computer<Pt>::profiler.active() &&
                           (graph_steps > 0 || last_key.n < YA_GRAPH_MAX_CELLS);
        const int n = read_n(!graph && sorted_pipeline_on());
        if (n <= 0) return;
        if constexpr (has_grid)
            if (graph && graph_step<pw_int, pw_friction>(n, dt, gen_forces)) return;
        heun_stages<pw_int, pw_friction>(n, dt, gen_forces);
        last_key = sorted_path ? key_of<pw_int, pw_friction>(n, dt) : Step_key{};  // (after the launches: they may have allocated)
    }

    // k steps in one call, bit for bit what k calls of take_step leave in d_X, d_old_v, d_n, d_dX, d_dX1 and
    // the grid's public arrays.  No model code runs between the steps of one call, so the id-ordered
    // arrays d_X / d_old_v -- the reference's contract BETWEEN two take_step calls -- need not exist in
    // between: Grid_solver's plain step (set_fixed(), no generic force) carries the cells in cube order.
    //   step 1, stage 1   the build by id, as take_step (n is read here, once)
    //   predictor         euler_step into a second entry buffer: d_sorted keeps {X0, id} in stage-1 order
    //   stage 2           rebuild from the predicted entries; the force kernel also leaves its right-hand
    //                     sides in ITS sorted order, k_order_from where each stage-1 slot went
    //   corrector         heun_step_sorted, per stage-1 slot -> {X, id}, {old_v, 0} in that order
    //   steps 2 .. k      stage 1 = rebuild from the corrector's output: k_order_from's rank count by id
    //                     restores ascending ids inside every cube, hence every sum's order
    //   step k            the corrector also stores d_X[id], d_old_v[id]
    // The centre-of-mass partial sums read d_dX / d_dX1 by id as ever (the force kernels' stores by id stay).
    // Nothing is remembered across calls: the next call's first build is by id again, so whatever a model
    // does between calls (copy_to_device, a kernel on d_X, another n) needs no invalidation.  Every
    // other configuration -- and k < 2 -- IS the loop of take_step.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(const float dt, const int k, Generic_forces<Pt> gen_forces)
    {
        if constexpr (has_grid)
            if (take_steps_carried<pw_int, pw_friction>(dt, k, gen_forces)) return;
        for (int s = 0; s < k; s++) take_step<pw_int, pw_friction>(dt, gen_forces);
    }
    // The update kernels of a carried call, one launch each.  Bin: the kernel bins the entries it stores (bin_in_update);
    // Tiles (four_tile_updates, with bin_in_update): its workgroups take so many tiles of UPDATE_BLOCK slots each, so
    // that the fold of the partial sums that each of them repeats runs in a quarter as many.
    template<typename F>
    void with_update_shape(F&& f) const
    {
        if (!bin_in_update) return f(std::false_type{}, std::integral_constant<int, 1>{});
        if (four_tile_updates) return f(std::true_type{}, std::integral_constant<int, 4>{});
        f(std::true_type{}, std::integral_constant<int, 1>{});
    }
    template<typename Bin, typename Tiles>
    void predict(Bin, Tiles, const int n, const float dt, const ya::Fix_args fix, const ya::Sorted_buffers<Pt>& at,
        const ya::Grid_bin bin)
    {
        constexpr int TILES = Tiles::value;
        const int wgs = (n + TILES * ya::UPDATE_BLOCK - 1) / (TILES * ya::UPDATE_BLOCK);
        euler_step<Pt, Fix::partials, Bin::value, TILES><<<wgs, ya::UPDATE_BLOCK, 0, this->stream>>>(n, dt, fix, d_dX, d_X,
            nullptr, at.rhs, at.cells, n, nullptr, nullptr, ya::Guard_band{}, at.carried, bin);
    }
    template<typename Bin, typename Tiles>
    void correct(Bin, Tiles, const int n, const float dt, const ya::Fix_args fix1, const ya::Sorted_buffers<Pt>& at,
        Pt* X_by_id, float3* v_by_id, const ya::Grid_bin bin)
    {
        constexpr int TILES = Tiles::value;
        const int wgs = (n + TILES * ya::UPDATE_BLOCK - 1) / (TILES * ya::UPDATE_BLOCK);
        heun_step_sorted<Pt, Bin::value, TILES><<<wgs, ya::UPDATE_BLOCK, 0, this->stream>>>(n, dt, d_mean_first, fix1, at.cells,
            at.rhs, at.carried_slots, at.carried_rhs, at.carried, at.carried_v, X_by_id, v_by_id, bin);
    }
    // false: does not qualify, nothing was done
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    bool take_steps_carried(const float dt, const int k, Generic_forces<Pt>& gen_forces)
    {
        if (!Computer<Pt>::carries || !carry_sorted || k < 2 || graph_steps != 0 || keep_order) return false;
        if (!update_folds_mean() || !ya::is_no_gen_forces<Pt>(gen_forces)) return false;
        if (!Computer<Pt>::carry_ready(n_max)) return false;  // (may allocate: before anything is queued)
        const int n = read_n(true);
        if (n <= 0) {  // nothing is carried, nothing is stale: the rest of the loop as it is
            for (int s = 1; s < k; s++) take_step<pw_int, pw_friction>(dt, gen_forces);
            return true;
        }
        // bin_in_update: every rebuild of the call (stage 2, and stage 1 of steps 2 .. k) bins the entries that
        // the update kernel in front of it has just stored, so that kernel bins them itself and the rebuild runs
        // without k_bin.  INVARIANT: the grid's count[] is zero between builds only because a scan follows every
        // binning (k_scan zeroes it in passing).  The predictor's binning is scanned by stage 2's rebuild, a
        // corrector's by the next step's stage 1 -- so the call's LAST corrector, behind which this call queues
        // no rebuild, must not bin.  The public point ids and the next build's visit order are read after the
        // call only: every rebuild but the last step's stage 2 leaves them unwritten (YA_REBUILD_PRIVATE).
        const bool fuse = bin_in_update;
        const ya::Grid_bin bin = fuse ? Computer<Pt>::bin_target() : ya::Grid_bin{};
        const unsigned quiet = fuse && trim_carried_stores ? YA_REBUILD_PRIVATE : 0u;
        const ya::Sorted_buffers<Pt> at = Computer<Pt>::sorted_buffers();
        for (int s = 0; s < k; s++) {
            const bool last = s == k - 1;
            int n_partials = 0;
            if (s == 0)
                Computer<Pt>::template pwints<pw_int, pw_friction>(n, d_X, d_old_v, d_dX, false, n, true);
            else
                Computer<Pt>::template pwints_carried<pw_int, pw_friction>(1, n, d_dX, fuse, quiet);
            YA_CHECK(ya_reduce_partials(d_dX, n_floats, n, d_workspace, &n_partials, this->stream));
            const ya::Fix_args fix{d_workspace, n_partials, d_mean_first};
            with_update_shape([&](auto binning, auto tiles) { predict(binning, tiles, n, dt, fix, at, bin); });
            Computer<Pt>::template pwints_carried<pw_int, pw_friction>(2, n, d_dX1, fuse, last ? 0u : quiet);
            YA_CHECK(ya_reduce_partials(d_dX1, n_floats, n, d_workspace, &n_partials, this->stream));
            const ya::Fix_args fix1{d_workspace, n_partials};
            with_update_shape([&](auto binning, auto tiles) {
                if (last)  // (the invariant above)
                    correct(std::false_type{}, tiles, n, dt, fix1, at, d_X, d_old_v, ya::Grid_bin{});
                else
                    correct(binning, tiles, n, dt, fix1, at, nullptr, nullptr, bin);
            });
        }
        if (fuse) fused_bin_rebuilds += 2 * k - 1;
        stage1_fix = d_mean_first;
        sorted_stage_cells = -1;
        rhs_zeroed[0] = rhs_zeroed[1] = 0;
        last_key = key_of<pw_int, pw_friction>(n, dt);
        carried_steps += k - 1;
        return true;
    }
};


// All-pairs interactions, LDS-tiled (solvers.cuh:279-342).  TILE_SIZE is kept
// for source compatibility; the kernel's own tile is ya::TILE_POINTS.
const auto TILE_SIZE = 32;

template<typename Pt>
class Tile_computer {
public:
    Tile_computer(int n_max) {}
    ya::Profiler profiler;
    static constexpr bool has_grid = false, carries = false;  // (what Heun_solver may ask of a computer)
    // 0 (default) = one thread owns a cell for the whole stage, as in the reference, unless the
    // functors are declared stateless (YA_STATELESS): then 64 lanes per cell up to 4096 cells and
    // 16 above; 1 = always one thread per cell; 16 or 64 = ya::tile_force_coop with that many
    // lanes per cell whatever the functor says (bit-identical sums; force launch at 800 cells
    // 196 -> 32 us with 64 lanes, at 3000 cells 631 -> 135 us with 16).
    int lanes_per_cell = 0;
    // Whether ya::tile_force_coop exists for Pt with 16 lanes per cell: 64 partners' terms for 16 cells must fit LDS,
    // which they do up to 10 floats (ya::tile_coop_partners).  Wider points get 64 lanes at every size when the
    // functors are stateless, and lanes_per_cell = 16 is refused for them at the first step.
    static constexpr bool has_16_lanes = ya::tile_coop_partners<Pt, 16>() >= 64;
    static_assert(ya::tile_coop_partners<Pt, 64>() >= 64, "64 lanes per cell fit LDS for every point of up to 16 floats");

protected:
    hipStream_t stream = nullptr;  // every launch of a step goes here (null = the default stream)
    using Step_variant = int;  // (no captured step: Heun_solver::Step_key)
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints(const int n, const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v,
        Pt* d_dX, const bool has_gen, const int n_active, const bool keep_sorted)
    {
        assert(n_active == n);  // Tile_solver is single-GPU only (all pairs)
        hipEvent_t start, stop;
        profiler.next(&start, &stop);
        int lanes = lanes_per_cell;
        if (lanes == 0)
            lanes = ya::stateless_pair<Pt, pw_int, pw_friction>() ? (n <= 4096 || !has_16_lanes ? 64 : 16) : 1;
        if (lanes >= 64)
            hipExtLaunchKernelGGL((ya::tile_force_coop<Pt, pw_int, pw_friction, 64>), dim3((n + 3) / 4),
                dim3(256), 0, stream, start, stop, 0, n, d_X, d_old_v, d_dX, has_gen);
        else if (lanes > 1) {
            if constexpr (has_16_lanes) {
                hipExtLaunchKernelGGL((ya::tile_force_coop<Pt, pw_int, pw_friction, 16>), dim3((n + 15) / 16),
                    dim3(256), 0, stream, start, stop, 0, n, d_X, d_old_v, d_dX, has_gen);
            } else {
                fprintf(stderr, "yalla-hip: Tile_computer::lanes_per_cell %d: points of %d floats have no 16-lane "
                                "kernel (a tile of their pair terms does not fit LDS); 0, 1 or 64\n", lanes,
                    ya::N_floats<Pt>::value);
                abort();
            }
        } else
            hipExtLaunchKernelGGL((ya::tile_force<Pt, pw_int, pw_friction>),
                dim3((n + ya::TILE_BLOCK - 1) / ya::TILE_BLOCK), dim3(ya::TILE_BLOCK), 0, stream, start,
                stop, 0, n, d_X, d_old_v, d_dX, has_gen);
    }
};

template<typename Pt>
using Tile_solver = Heun_solver<Pt, Tile_computer>;


// Uniform grid over space: cells sorted by cube id, ONLY points closer than
// cube_size interact (solvers.cuh:345-425).  The four arrays and the device
// mirror d_grid are public API used from model kernels, e.g.
// `d_grid->d_cube_start[cube]`.
class Grid {
public:
    int *d_cube_id, *d_point_id, *d_cube_start, *d_cube_end;
    Grid* d_grid;
    const int n_max, grid_size, n_cubes;
    Grid(int n_max, int gs = 50) : n_max{n_max}, grid_size{gs}, n_cubes{gs * gs * gs}
    {
        YA_CHECK(ya_grid_create(n_max, gs, &handle));
        YA_CHECK(ya_grid_arrays(handle, &d_cube_id, &d_point_id, &d_cube_start, &d_cube_end));
        YA_CHECK(ya_grid_offsets(handle, &d_offs));
        YA_CHECK(ya_malloc((void**)&d_grid, sizeof(Grid)));
        YA_CHECK(ya_memcpy_h2d(d_grid, this, sizeof(Grid)));
    }
    ~Grid()
    {
        ya_free(d_grid);
        ya_grid_destroy(handle);
    }
    Grid(const Grid&) = delete;
    template<typename Pt>
    void build(const int n, const Pt* __restrict__ d_X, const float cube_size = 1)
    {
        YA_CHECK(ya_grid_build(handle, d_X, sizeof(Pt), n, cube_size, nullptr));
    }
    template<typename Pt, template<typename> class Solver>
    void build(Solution<Pt, Solver>& points, const float cube_size = 1)
    {
        auto n = points.get_d_n();
        assert(n <= n_max);
        build(n, points.d_X, cube_size);
    }
    // Engine-side extras (not in the reference).
    template<typename Pt>
    void build_sorted(const int n, const Pt* d_X, const float3* d_old_v, const float cube_size,
        ya::Entry<Pt>* d_sorted, float4* d_sorted_v, hipStream_t stream = nullptr)
    {
        YA_CHECK(ya_grid_build_sorted(handle, d_X, sizeof(Pt), d_old_v, n, cube_size, d_sorted,
            sizeof(ya::Entry<Pt>), d_sorted_v, stream));
    }
    // build_sorted in two halves: the first one reads the count on the device and can be
    // queued before the host has it (ya_grid_build_sorted_begin / _finish).
    template<typename Pt>
    void build_sorted_begin(const Pt* d_X, const int* d_n, const int n_bound, const float cube_size, ya_n_reader* reader)
    {
        YA_CHECK(ya_grid_build_sorted_begin_publish(handle, d_X, sizeof(Pt), d_n, n_bound, cube_size, reader, nullptr));
    }
    template<typename Pt>
    void build_sorted_finish(const int n, const Pt* d_X, const float3* d_old_v,
        ya::Entry<Pt>* d_sorted, float4* d_sorted_v)
    {
        YA_CHECK(ya_grid_build_sorted_finish(handle, d_X, sizeof(Pt), d_old_v, n, d_sorted,
            sizeof(ya::Entry<Pt>), d_sorted_v, nullptr));
    }
    // Same result as build_sorted on the cells held (in any order) by d_prev, read
    // from those entries themselves: nothing is gathered through point ids.
    template<typename Pt>
    void rebuild_sorted(const int n, const ya::Entry<Pt>* d_prev, const float4* d_prev_v,
        const float cube_size, ya::Entry<Pt>* d_sorted, float4* d_sorted_v,
        hipStream_t stream = nullptr, int* d_slot_of_prev = nullptr)
    {
        YA_CHECK(ya_grid_rebuild_sorted_map(handle, d_prev, sizeof(ya::Entry<Pt>), sizeof(Pt),
            d_prev_v, n, cube_size, d_sorted, d_sorted_v, d_slot_of_prev, stream));
    }
    // rebuild_sorted without its binning launch, for entries that the caller's own kernels have binned
    // (ya::bin_entry into bin_target()) since this grid's last build: exactly these n, each once, in storage order,
    // with this cube size (ya_grid_rebuild_sorted_binned's precondition).  flags: YA_REBUILD_*.
    template<typename Pt>
    void rebuild_sorted_binned(const int n, const ya::Entry<Pt>* d_prev, const float4* d_prev_v,
        const float cube_size, ya::Entry<Pt>* d_sorted, float4* d_sorted_v, hipStream_t stream, int* d_slot_of_prev,
        const unsigned flags)
    {
        YA_CHECK(ya_grid_rebuild_sorted_binned(handle, d_prev, sizeof(ya::Entry<Pt>), sizeof(Pt), d_prev_v, n,
            cube_size, d_sorted, d_sorted_v, d_slot_of_prev, flags, stream));
    }
    ya_grid_bin_target bin_target()
    {
        ya_grid_bin_target t{};
        YA_CHECK(ya_grid_bin_target_get(handle, &t));
        return t;
    }
    const int* offsets() const { return d_offs; }
    // The ids the last build saw mean other cells now (Solution::renumber): the next build visits
    // the cells in storage order instead of the last build's.
    void forget_order() { YA_CHECK(ya_grid_forget_order(handle)); }
    // A promise that every cell's cube id lies in [cube_lo, cube_hi): builds then scan those cubes
    // only (ya_grid_set_cube_range; a z-slab holds cells in a fraction of the grid's planes).
    void set_cube_range(const int cube_lo, const int cube_hi) { YA_CHECK(ya_grid_set_cube_range(handle, cube_lo, cube_hi)); }
    void check_status()
    {
        int bits = 0;
        YA_CHECK(ya_grid_status(handle, &bits, 1));
        if (bits & YA_STATUS_OUT_OF_RANGE) {
            fprintf(stderr,
                "yalla-hip: a cell left the cube range its z-slab promised the grid (Grid::set_cube_range): it "
                "moved more than a cube between two selections of the mirrored cells.\n");
            abort();
        }
        if (bits & YA_STATUS_SCAN_STALLED) {
            fprintf(stderr,
                "yalla-hip: the grid build's prefix sum stalled (a workgroup waited for one of lower index that had "
                "not been started: the device does not dispatch workgroups in index order, or two builds of one "
                "Grid ran at once on different streams).  The grid arrays of that build are not valid.\n");
            abort();
        }
        if (bits & YA_STATUS_OUT_OF_GRID) {
            fprintf(stderr,
                "yalla-hip: a cell left the %d^3 grid (device assertion at "
                "ya||a solvers.cuh:361-362); enlarge grid_size or cube_size.\n",
                grid_size);
            abort();
        }
    }

private:
    ya_grid* handle = nullptr;
    const int* d_offs = nullptr;
};


__constant__ int d_nhood[27];  // stencil offsets for model kernels (solvers.cuh:428)

enum Ya_sum_order { YA_SUM_REFERENCE = 0, YA_SUM_BY_PLANE = 1 };  // Grid_computer::sum_order

namespace ya {
// One launch of a force kernel.  A timed launch (start given) carries its events in the dispatch itself
// (ya::Profiler); an untimed one is a plain launch, which is also what a stream capture records.
template<typename... Params, typename... Args>
void launch(void (*kernel)(Params...), const dim3 grid, const dim3 block, hipStream_t stream, hipEvent_t start,
    hipEvent_t stop, Args... args)
{
    if (start)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, start, stop, 0, static_cast<Params>(args)...);
    else
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<Params>(args)...);
}
// The runtime-to-template choices of the grid force launches, each written once: f is a generic lambda that is handed
// the choice as std::integral_constant values.  Exactly these combinations are built, no others.
namespace coop {
template<typename F>
bool with_lanes(const int lanes, F&& f)  // false: not a grid_force_coop launch
{
    if (lanes == 16) return f(std::integral_constant<int, 16>{}), true;
    if (lanes == 8) return f(std::integral_constant<int, 8>{}), true;
    if (lanes == 4) return f(std::integral_constant<int, 4>{}), true;
    return false;
}
}  // namespace coop
namespace bits {
// (STAGE_V, OFF32): old_v from LDS, where every offset fits 32 bits; else from global memory through 32-bit byte
// offsets while 16 n fits them, through 64-bit addresses beyond
template<typename F>
void with_gather(const bool stage_v, const bool off32, F&& f)
{
    if (stage_v) return f(std::true_type{}, std::true_type{});
    if (off32) return f(std::false_type{}, std::true_type{});
    f(std::false_type{}, std::false_type{});
}
// The shape of one grid_force_bits launch of n cells, pure arithmetic: Grid_computer::forces launches by it, and
// Grid_computer::ready_to_capture asks the same function.
// HALF TILES ("the tail"; tail > 0: the last so many tiles of the launch, < 0: all, 0: none).  With R = `resident`
// one-wavefront workgroups on the chip at once (5120 for springs): launches of up to R / 2 tiles are made of halves
// altogether; up to R tiles, as many tiles are split as fill the chip in its one round (R - tiles); beyond, the launch
// ends with 768 tiles as halves (measured at 2 * 10^5 ... 10^7 cells, profiles/r05_tail_ab.txt).  A slab stage's two
// launches (part 1 / 2) run side by side: all halves only if both fit at once; the kernel leaves a list of < 4 tails'
// tiles whole.  Two wavefronts then call the functor for the same cell i at once: only for functors declared stateless
// (YA_STATELESS; relu_w_epithelium's `d_mes_nbs[i] += 1` would lose counts), and only summing by plane.
struct Plan_settings {
    bool by_plane, stateless;                         // Grid_computer::sum_order, ya::stateless_pair
    int tail_tiles, stage_v_max, gather_offset_bits;  // Grid_computer::force_tail_tiles, ...
    bool tail_by_residency() const { return by_plane && stateless && tail_tiles < 0; }  // else `resident` is not read
};
struct Plan {
    int tiles, tail, room, blocks;  // room: exchange slots the tail needs; blocks: workgroups launched
    bool stage_v, off32;
    bool fits(const int tail_room) const { return room <= tail_room; }  // no exchange area has to be allocated
};
inline Plan plan(const int n, const int part, const int resident, const Plan_settings& s)
{
    Plan p{};
    p.tiles = (n + BLOCK - 1) / BLOCK;
    if (!s.by_plane || !s.stateless)
        p.tail = 0;
    else if (s.tail_tiles >= 0)
        p.tail = s.tail_tiles >= p.tiles ? -1 : s.tail_tiles;
    else if (2 * p.tiles <= resident)
        p.tail = -1;
    else
        p.tail = part == 0 && p.tiles <= resident ? resident - p.tiles : 768;
    p.room = p.tail < 0 ? p.tiles : p.tail;
    p.blocks = p.tail < 0 ? 16 * ((p.tiles + 7) / 8) : p.tiles + (p.tail > 0 ? std::min(p.tail, p.tiles) + 24 : 0);
    // (old_v in LDS costs a launch of halves the residency it lives on: 13 KB per workgroup are 12 per CU)
    p.stage_v = n <= s.stage_v_max && p.tail >= 0;
    p.off32 = s.gather_offset_bits != 64 && offsets_fit_32_bits(n);
    return p;
}
}  // namespace bits
}  // namespace ya

template<typename Pt>
class Grid_computer {
public:
    float cube_size;
    ya::Profiler profiler;
    // 2 = grid_force_bits (bit stream) always; 1 = grid_force (byte FIFO), 0 = grid_force_direct: the A/B
    // baselines of tools/ab/force_variants.cuh, only with -DYA_EXPERIMENTAL_FORCE_VARIANTS;
    // 3 = grid_force_coop below ~7 * 10^4 cells (16, 8 or 4 lanes per cell, more the smaller the
    // system), grid_force_bits above: for models whose functors keep no per-cell state without
    // atomics (bit-identical results; see the kernel's comment)
    // -1 (default) = grid_force_bits, or -- for functors declared stateless (YA_STATELESS) --
    // grid_force_coop below ~7 * 10^4 cells
    int force_variant = -1;
    // The order in which a cell's pair terms are added (both restated in oracle/yalla_host.hpp under the same names):
    //   YA_SUM_REFERENCE (default)  one running sum over the 27 cubes in d_nhood order -- the reference's
    //                               thread (solvers.cuh:437-459), bit for bit for + - * / sqrt fma functors;
    //   YA_SUM_BY_PLANE  (opt-in)   S[own z-plane] + S[planes below and above], each in the reference's order:
    //                               lets grid_force_bits give a tile's planes to two wavefronts ("the tail";
    //                               launches of 7 * 10^4 .. 1.6 * 10^5 cells as halves altogether).  ~1e-7
    //                               relative per step beside the reference's sum, inside north_star's 1e-5.
    Ya_sum_order sum_order = YA_SUM_REFERENCE;
    int coop_lanes = 0;            // force_variant 3: 0 = from n (ya::coop::lanes_for), or 4 / 8 / 16
    int stage_v_max = 130000;      // grid_force_bits keeps old_v in LDS too up to this many cells
    // grid_force_bits gathers old_v through 32-bit byte offsets while 16 n fits them (ya::bits::offsets_fit_32_bits)
    // and builds 64-bit addresses beyond: 0 = by n, 64 = the 64-bit form at any size (A/B, tests; same results)
    int gather_offset_bits = 0;
    // grid_force_bits: what a pass may know about its hits before phase 2 (ya::bits::launch_facts): 1 (default) = no
    // self pair where the pass' rows cannot hold the lane's own slot, and dist < 1 for every hit while cube_size <= 1
    // (exact tier); 0 = the generic bodies only; 2 / 3 = the first / the second fact alone (A/B).  Same results.
    int pass_facts = 1;
    // (Heun_solver's traits; use_sorted_pipeline() and carry_ready() say when the cells are kept cube-sorted)
    static constexpr bool has_grid = true, carries = true;
    Grid_computer(int n_max, int grid_size = 50, float cube_size = 1)
        : cube_size{cube_size}, grid{n_max, grid_size}
    {
        // Row-major 3x3x3 offsets in the order x, then {0,-gs,+gs}, then
        // {0,-gs^2,+gs^2} (solvers.cuh:472-483).
        int h_nhood[27];
        const int shift[3] = {0, -1, 1};
        for (int z = 0; z < 3; z++)
            for (int y = 0; y < 3; y++)
                for (int x = 0; x < 3; x++)
                    h_nhood[9 * z + 3 * y + x] =
                        (x - 1) + shift[y] * grid_size + shift[z] * grid_size * grid_size;
        YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(d_nhood), h_nhood, sizeof(h_nhood)));
        YA_CHECK(ya_malloc((void**)&d_sorted, (size_t)n_max * sizeof(ya::Entry<Pt>)));
        YA_CHECK(ya_malloc((void**)&d_sorted_v, (size_t)n_max * sizeof(float4)));
        YA_CHECK(ya_malloc((void**)&d_resorted, (size_t)n_max * sizeof(ya::Entry<Pt>)));
        YA_CHECK(ya_malloc((void**)&d_resorted_v, (size_t)n_max * sizeof(float4)));
        YA_CHECK(ya_malloc((void**)&d_dX_sorted, (size_t)n_max * sizeof(Pt)));
    }
    ~Grid_computer()
    {
        ya_free(d_sorted);
        ya_free(d_sorted_v);
        ya_free(d_resorted);
        ya_free(d_resorted_v);
        ya_free(d_dX_sorted);
        if (d_carried) ya_free(d_carried), ya_free(d_carried_rhs), ya_free(d_carried_slots);
        for (int p = 0; p < 3; p++) ya_free(d_tail_exchange[p]), ya_free(d_tail_tickets[p]);
        if (interior_stream && interior_stream_owned) (void)hipStreamDestroy(interior_stream);
        if (grid_built) {
            (void)hipEventDestroy(grid_built);
            (void)hipEventDestroy(interior_done);
        }
    }
    Grid_computer(const Grid_computer&) = delete;
    // grid_force_bits' tail (the last tiles of a launch as half tiles): -1 = chosen from the launch's size,
    // 0 = none, or the number of tiles (A/B knob).  Results do not depend on it.
    int force_tail_tiles = -1;  // (a number of the launch's tiles or more: every tile as halves)
    float* d_tail_exchange[3] = {nullptr, nullptr, nullptr};  // per launch kind (part 0 / 1 / 2)
    int* d_tail_tickets[3] = {nullptr, nullptr, nullptr};
    int tail_room[3] = {0, 0, 0};
    // one-wavefront workgroups of `Kernel` the CURRENT device holds at once (occupancy x CUs), per device
    template<auto Kernel>
    static int resident_workgroups()
    {
        static std::mutex lock;
        static std::vector<int> by_device;
        int device = 0;
        YA_CHECK((int)hipGetDevice(&device));
        std::lock_guard<std::mutex> hold(lock);
        if ((int)by_device.size() <= device) by_device.resize(device + 1, 0);
        if (by_device[device] == 0) {
            int per_cu = 0, cus = 0;
            YA_CHECK((int)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, ya::bits::BLOCK, 0));
            YA_CHECK((int)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
            by_device[device] = per_cu * cus;
        }
        return by_device[device];
    }
    bool sorted_pipeline = true;  // false = both stages through d_X / d_X1 (A/B)
    // z-slab decomposition (include/slab_logic.inc): 1 = the next forces() call launches the tiles
    // in the z-planes next to the slab's faces only (cube ids below force_part_cube_lo or from
    // force_part_cube_hi up) and remembers its arguments; forces_interior() then launches the
    // rest on a stream of its own, and join_interior() makes the step's stream wait for it.  The
    // exchange of the boundary cells' right-hand sides runs beside the interior launch.  Kernels
    // other than grid_force_bits compute everything in the first call.
    int force_part = 0;
    int force_part_cube_lo = 0, force_part_cube_hi = 0x7fffffff;
    // ... and the cubes that can hold own cells at all: [force_own_cube_lo, force_own_cube_hi); tiles of
    // cubes outside hold mirrored cells only and are left out of both launches
    int force_own_cube_lo = 0, force_own_cube_hi = 0x7fffffff;
    // z-slab decomposition: local cell index -> global id (own cells, then ghosts); pairwise
    // functors are then called with global (i, j).  NULL (default): local = global.
    const int* d_global_id = nullptr;
    bool use_sorted_pipeline() const { return sorted_pipeline and force_variant != 0; }

protected:
    hipStream_t stream = nullptr;  // every launch of a step goes here (null = the default stream)
    // Everything of this class that a captured step bakes into its launches (Heun_solver::Step_key compares it
    // at every step: the members are public and assigned directly).  A member added to forces() that picks a
    // kernel, a launch size or a kernel argument belongs here too.
    struct Step_variant {
        int force_variant = -1, sum_order = 0, coop_lanes = 0, stage_v_max = 0, tail_tiles = 0, gather_offset_bits = 0;
        int pass_facts = 1;
        int tail_areas = 0;  // allocations of tail exchange areas so far: a graph made before one holds freed pointers
        const int* global_id = nullptr;
        auto tied() const
        {
            return std::tie(force_variant, sum_order, coop_lanes, stage_v_max, tail_tiles, gather_offset_bits, pass_facts,
                tail_areas, global_id);
        }
        bool operator==(const Step_variant& o) const { return tied() == o.tied(); }
    };
    Step_variant step_variant() const
    {
        return {force_variant, (int)sum_order, coop_lanes, stage_v_max, force_tail_tiles, gather_offset_bits, pass_facts,
            tail_areas, d_global_id};
    }
    int tail_areas = 0;
    Grid grid;
    ya::Entry<Pt>*d_sorted, *d_resorted;
    float4 *d_sorted_v, *d_resorted_v;
    Pt* d_dX_sorted;
    void check_status() { grid.check_status(); }
    struct Forces_call {
        int n = 0, n_active = 0;
        const ya::Entry<Pt>* d_cells = nullptr;
        const float4* d_cells_v = nullptr;
        Pt *d_dX = nullptr, *d_dX_in_cell_order = nullptr;
        bool has_gen = false, split = false;
    } boundary_call;
    hipStream_t interior_stream = nullptr;
    bool interior_stream_owned = false;
    hipEvent_t grid_built = nullptr, interior_done = nullptr;
    // The stream of a stage's second force launch, supplied by the program (several solvers of
    // one process may share one: every stream beyond the device's few hardware queues shares a
    // queue with another, and two launches on one queue run one after the other).  Call before
    // the first decomposed step; the stream stays the caller's.
    void use_interior_stream(hipStream_t s)
    {
        if (interior_stream && interior_stream_owned) (void)hipStreamDestroy(interior_stream);
        interior_stream = s;
        interior_stream_owned = false;
    }
    // the second launch of a stage whose first one ran with force_part = 1
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces_interior()
    {
        if (!boundary_call.split) return;  // the first call computed every tile
        const Forces_call c = boundary_call;
        const int part = force_part;
        force_part = 2;
        forces<pw_int, pw_friction>(c.n, c.d_cells, c.d_cells_v, c.d_dX, c.has_gen, c.n_active, c.d_dX_in_cell_order);
        force_part = part;
        YA_CHECK((int)hipEventRecord(interior_done, interior_stream));
    }
    void join_interior()
    {
        if (!boundary_call.split) return;
        YA_CHECK((int)hipStreamWaitEvent(stream, interior_done, 0));
        boundary_call.split = false;
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces(const int n, const ya::Entry<Pt>* d_cells, const float4* d_cells_v, Pt* d_dX,
        const bool has_gen, const int n_active, Pt* d_dX_in_cell_order)
    {
        hipEvent_t start, stop;
        profiler.next(&start, &stop);
        const float cut2 = ya::cutoff_squared(cube_size);
        const bool by_plane = sum_order == YA_SUM_BY_PLANE;
        // the kernel this launch goes to: an explicit choice, or by what the model said about its functors
        const Kernel_choice choice = kernel_choice<pw_int, pw_friction>(n);
        if (choice.variant < 0 || choice.variant > 3) {
            fprintf(stderr, "yalla-hip: Grid_computer::force_variant %d is not a kernel (-1, 0, 1, 2, 3)\n", choice.variant);
            abort();
        }
        const int part = slab_part({n, n_active, d_cells, d_cells_v, d_dX, d_dX_in_cell_order, has_gen, choice.bits_kernel()});
        hipStream_t stream = part == 2 ? interior_stream : this->stream;
        const bool coop = ya::coop::with_lanes(choice.lanes, [&](auto lanes) {
            constexpr int CELLS = ya::coop::BLOCK / decltype(lanes)::value;
            ya::launch(ya::grid_force_coop<Pt, pw_int, pw_friction, decltype(lanes)::value>, (n + CELLS - 1) / CELLS,
                ya::coop::BLOCK, stream, start, stop, n, d_cells, d_cells_v, grid.d_cube_id, grid.offsets(),
                grid.grid_size, grid.n_cubes, cut2, d_dX, has_gen, n_active, d_dX_in_cell_order, d_global_id, by_plane);
        });
        if (coop) return;
        if (choice.variant >= 2) {
            const ya::bits::Plan plan = bits_plan<pw_int, pw_friction>(n, part);
            ensure_tail_room<pw_int, pw_friction>(part, plan.room);
            const auto launch_bits = [&](auto global_ids) {
                ya::bits::with_gather(plan.stage_v, plan.off32, [&](auto stage_v, auto off32) {
                    ya::launch(ya::grid_force_bits<Pt, pw_int, pw_friction, decltype(stage_v)::value,
                                   decltype(global_ids)::value, decltype(off32)::value>,
                        plan.blocks, ya::bits::BLOCK, stream, start, stop, n, d_cells, d_cells_v, grid.d_cube_id,
                        grid.offsets(), grid.grid_size, grid.n_cubes, cut2, d_dX, has_gen, n_active, d_dX_in_cell_order,
                        d_global_id, plan.tiles, plan.tail, d_tail_exchange[part], d_tail_tickets[part], by_plane, part,
                        force_part_cube_lo, force_part_cube_hi, force_own_cube_lo, force_own_cube_hi,
                        ya::bits::launch_facts(pass_facts, cut2));
                });
            };
            return d_global_id ? launch_bits(std::true_type{}) : launch_bits(std::false_type{});
        }
#ifdef YA_EXPERIMENTAL_FORCE_VARIANTS
        const int blocks = (n + ya::FORCE_BLOCK - 1) / ya::FORCE_BLOCK;
        if (choice.variant == 0)
            ya::launch(ya::grid_force_direct<Pt, pw_int, pw_friction>, blocks, ya::FORCE_BLOCK, stream, start, stop, n,
                d_cells, d_cells_v, grid.d_cube_id, grid.offsets(), grid.grid_size, grid.n_cubes, cube_size, d_dX,
                has_gen, n_active, d_global_id, by_plane);
        else
            ya::launch(ya::grid_force<Pt, pw_int, pw_friction>, blocks, ya::FORCE_BLOCK, stream, start, stop, n, d_cells,
                d_cells_v, grid.d_cube_id, grid.offsets(), grid.grid_size, grid.n_cubes, cut2, d_dX, has_gen, n_active,
                d_dX_in_cell_order, d_global_id, by_plane);
#else
        fprintf(stderr, "yalla-hip: Grid_computer::force_variant %d is an A/B baseline kept in "
                        "tools/ab/force_variants.cuh: compile with -DYA_EXPERIMENTAL_FORCE_VARIANTS -Itools/ab\n", choice.variant);
        abort();
#endif
    }
    // A z-slab's stage as two launches (force_part; what grid_force_bits offers -- the other kernels compute every tile
    // in the first call): which part the launch of `call` is -- 0 the whole stage, 1 the tiles next to the slab's faces,
    // 2 the rest -- with what orders part 2, on its own stream, behind the grid build and not behind part 1.
    int slab_part(const Forces_call& call)
    {
        if (force_part == 1) {
            boundary_call = call;
            if (call.split) {
                if (!interior_stream) {
                    // YA_INTERIOR_LOW_PRIORITY=1: the boundary launch, whose rows the neighbours
                    // wait for, gets the chip first.  Measured in the one-GPU rehearsal (10 M cells,
                    // 8 slabs): the boundary rows are ready after 173-210 instead of 255 us, but the
                    // interior launch then starts 110 us late and the stage takes 333 instead of
                    // 312 us -- off by default until a real neighbour has been seen waiting.
                    int least = 0, greatest = 0;
                    YA_CHECK((int)hipDeviceGetStreamPriorityRange(&least, &greatest));
                    YA_CHECK((int)hipStreamCreateWithPriority(&interior_stream, hipStreamNonBlocking,
                        getenv("YA_INTERIOR_LOW_PRIORITY") ? least : 0));
                    interior_stream_owned = true;
                }
                if (!grid_built) {
                    YA_CHECK((int)hipEventCreateWithFlags(&grid_built, hipEventDisableTiming));
                    YA_CHECK((int)hipEventCreateWithFlags(&interior_done, hipEventDisableTiming));
                }
                // the interior launch needs the grid, not the boundary launch
                YA_CHECK((int)hipEventRecord(grid_built, stream));
                return 1;
            }
        } else if (force_part == 2) {
            YA_CHECK((int)hipStreamWaitEvent(interior_stream, grid_built, 0));
            return 2;
        }
        return 0;
    }
    // Room for `room` half tiles' sums in part's exchange area (a solver's launches are stream-ordered except parts 1
    // and 2 of a slab stage, which have exchange areas of their own).
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void ensure_tail_room(const int part, const int room)
    {
        if (room <= tail_room[part]) return;
        constexpr int NC = ya::N_floats<Pt>::value + 4;
        // Never inside a stream capture: Heun_solver::take_step captures a step only after the same step
        // ran plainly (which came through here) and after ready_to_capture() said nothing is missing.
        // Should a new path get here all the same, say what happened instead of a bare HIP error code.
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (this->stream) YA_CHECK((int)hipStreamIsCapturing(this->stream, &capturing));
        if (capturing != hipStreamCaptureStatusNone) {
            fprintf(stderr, "yalla-hip: grid_force_bits' tail exchange area would have to be allocated inside a "
                            "stream capture (Grid_computer::ready_to_capture missed a case)\n");
            abort();
        }
        YA_CHECK(ya_device_synchronize());
        if (d_tail_exchange[part]) ya_free(d_tail_exchange[part]), ya_free(d_tail_tickets[part]);
        // once per solver, not once per size: a system that grows (proliferation) asks for a tile more
        // every few steps while its launches are made of halves, which they are up to `resident` tiles
        const int most = std::min((grid.n_max + ya::bits::BLOCK - 1) / ya::bits::BLOCK,
            std::max(resident_workgroups<ya::grid_force_bits<Pt, pw_int, pw_friction, false, false>>(), 768));
        const size_t slots = (size_t)std::max(room, most) + 8;
        YA_CHECK(ya_malloc((void**)&d_tail_exchange[part], slots * 2 * NC * ya::bits::BLOCK * sizeof(float)));
        YA_CHECK(ya_malloc((void**)&d_tail_tickets[part], slots * sizeof(int)));
        YA_CHECK(ya_memset_async(d_tail_tickets[part], 0, slots * sizeof(int), nullptr));
        YA_CHECK(ya_device_synchronize());
        tail_room[part] = (int)slots - 8;
        tail_areas++;  // (graphs captured so far hold the freed areas' addresses: Step_variant)
    }
    // The kernel a launch of n cells goes to (forces() and ready_to_capture()): an explicit choice, or by what the
    // model said about its functors; lanes per cell (1: not grid_force_coop)
    struct Kernel_choice {
        int variant, lanes;
        bool bits_kernel() const { return lanes == 1 && variant >= 2; }  // grid_force_bits: tails, two launches per stage
    };
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    Kernel_choice kernel_choice(const int n) const
    {
        const int variant = force_variant >= 0 ? force_variant : (ya::stateless_pair<Pt, pw_int, pw_friction>() ? 3 : 2);
        const int lanes =
            variant == 3 ? (coop_lanes ? coop_lanes : ya::coop::lanes_for(n, sum_order == YA_SUM_BY_PLANE)) : 1;
        return {variant, lanes};
    }
    // ya::bits::plan of this computer's settings; the occupancy is asked for only where the plan reads it
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    ya::bits::Plan bits_plan(const int n, const int part) const
    {
        const ya::bits::Plan_settings s{sum_order == YA_SUM_BY_PLANE, ya::stateless_pair<Pt, pw_int, pw_friction>(),
            force_tail_tiles, stage_v_max, gather_offset_bits};
        constexpr auto kernel = ya::grid_force_bits<Pt, pw_int, pw_friction, false, false>;
        return ya::bits::plan(n, part, s.tail_by_residency() ? resident_workgroups<kernel>() : 0, s);
    }
    // Heun_solver::take_step before it captures a step of n cells: would forces() have to allocate?  (The captured
    // step is an undivided one: part 0.)
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    bool ready_to_capture(const int n) const
    {
        return !kernel_choice<pw_int, pw_friction>(n).bits_kernel() || bits_plan<pw_int, pw_friction>(n, 0).fits(tail_room[0]);
    }
    // Heun_solver::renumber: the cells' ids in (cube, id) order = the point ids of a fresh build
    const int* cube_order(const int n, const Pt* d_X)
    {
        grid.build(n, d_X, cube_size);
        return grid.d_point_id;
    }
    // ... after which cell s IS slot s: the next build visits the cells in storage order
    void ids_changed() { grid.forget_order(); }
    // The part of the first stage's grid build that can be queued before the host knows
    // n (Heun_solver::take_step); pwints then only finishes the build.
    void begin_build(const Pt* d_X, const int* d_n, const int n_bound, ya_n_reader* reader)
    {
        grid.build_sorted_begin(d_X, d_n, n_bound, cube_size, reader);
        build_begun = true;
    }
    void cancel_build() { build_begun = false; }
    bool build_begun = false;
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints(const int n, const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v,
        Pt* d_dX, const bool has_gen, const int n_active, const bool keep_sorted)
    {
        if (build_begun)
            grid.build_sorted_finish(n, d_X, d_old_v, d_sorted, d_sorted_v);
        else
            grid.build_sorted(n, d_X, d_old_v, cube_size, d_sorted, d_sorted_v, stream);
        build_begun = false;
        forces<pw_int, pw_friction>(n, d_sorted, d_sorted_v, d_dX, has_gen, n_active,
            keep_sorted ? d_dX_sorted : nullptr);
    }
    // (the corrector's {old_v, 0} go to d_resorted_v, dead after stage 2's force launch)
    ya::Sorted_buffers<Pt> sorted_buffers()
    {
        return {d_sorted, d_dX_sorted, d_carried, d_resorted_v, d_carried_rhs, d_carried_slots};
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints_from_sorted(const int n, Pt* d_dX, const int n_active, const bool has_gen)
    {
        grid.rebuild_sorted(n, d_sorted, d_sorted_v, cube_size, d_resorted, d_resorted_v, stream);
        forces<pw_int, pw_friction>(n, d_resorted, d_resorted_v, d_dX, has_gen, n_active, nullptr);
    }
    // ---- cells carried in cube order from step to step (Heun_solver::take_steps) ----
    // Buffers beyond a plain step's, ~32 bytes per cell, made by the first call that carries:
    //   d_carried        entries: the predictor's output, then -- dead once stage 2 is built -- the corrector's
    //   d_carried_rhs    stage 2's right-hand sides in stage 2's sorted order
    //   d_carried_slots  stage-1 slot -> stage-2 slot
    ya::Entry<Pt>* d_carried = nullptr;
    Pt* d_carried_rhs = nullptr;
    int* d_carried_slots = nullptr;
    // Does this computer carry right now (undivided, local ids = global ids), and has it the memory?  Called
    // outside any stream capture, before the call's first launch; false = the plain loop.
    bool carry_ready(const int n_max)
    {
        if (!use_sorted_pipeline() || d_global_id || force_part != 0) return false;
        if (d_carried) return true;
        if (carry_refused) return false;
        const int rc[3] = {ya_malloc((void**)&d_carried, (size_t)n_max * sizeof(ya::Entry<Pt>)),
            ya_malloc((void**)&d_carried_rhs, (size_t)n_max * sizeof(Pt)),
            ya_malloc((void**)&d_carried_slots, (size_t)n_max * sizeof(int))};
        if (rc[0] == 0 && rc[1] == 0 && rc[2] == 0) return true;
        // out of memory: the plain loop needs none of it (and the runtime's sticky-free error is taken off)
        if (rc[0] == 0) ya_free(d_carried);
        if (rc[1] == 0) ya_free(d_carried_rhs);
        if (rc[2] == 0) ya_free(d_carried_slots);
        d_carried = nullptr, d_carried_rhs = nullptr, d_carried_slots = nullptr;
        (void)hipGetLastError();
        carry_refused = true;  // (not asked for again at every call)
        return false;
    }
    bool carry_refused = false;
    // stage 1 of a carried step after the call's first: from the corrector's output, as stage 2 starts from
    // the predictor's; stage 2: from the predicted entries, with the slot map and the sorted right-hand sides
    // binned: the update kernel in front has binned d_carried's entries into bin_target() with this cube size
    // (Grid::rebuild_sorted_binned's precondition); flags: YA_REBUILD_*
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints_carried(const int stage, const int n, Pt* d_dX, const bool binned, const unsigned flags)
    {
        const float4* prev_v = stage == 1 ? d_resorted_v : d_sorted_v;
        ya::Entry<Pt>* out = stage == 1 ? d_sorted : d_resorted;
        float4* out_v = stage == 1 ? d_sorted_v : d_resorted_v;
        int* slots = stage == 1 ? nullptr : d_carried_slots;
        if (binned)
            grid.rebuild_sorted_binned(n, d_carried, prev_v, cube_size, out, out_v, stream, slots, flags);
        else
            grid.rebuild_sorted(n, d_carried, prev_v, cube_size, out, out_v, stream, slots);
        forces<pw_int, pw_friction>(n, out, out_v, d_dX, false, n, stage == 1 ? d_dX_sorted : d_carried_rhs);
    }
    // where the update kernels of a carried step bin (the cube size is the one the rebuilds are given)
    ya::Grid_bin bin_target() { return ya::Grid_bin{grid.bin_target(), cube_size}; }
};

template<typename Pt>
using Grid_solver = Heun_solver<Pt, Grid_computer>;


// Pairwise interactions on the grid restricted to Gabriel-graph neighbours
// (Delile et al. 2017, Marin-Riera et al. 2016; solvers.cuh:505-644).
template<typename Pt>
class Gabriel_computer : public Grid_computer<Pt> {
public:
    float gabriel_coefficient;
    // -1 (default) = ya::gabriel_force (+ ya::gabriel_force_dense for cells with more than GABRIEL_CAP
    // candidates); 0 = gabriel_force_direct, the A/B baseline of tools/ab/force_variants.cuh, only with
    // -DYA_EXPERIMENTAL_FORCE_VARIANTS (at most 100 candidates per cell).  (Grid_computer::force_variant.)
    Gabriel_computer(
        int n_max, int grid_size = 50, float cube_size = 1, float gabriel_coefficient = 0.8)
        : Grid_computer<Pt>{n_max, grid_size, cube_size}, gabriel_coefficient{gabriel_coefficient}
    {
        YA_CHECK(ya_malloc((void**)&d_dense, (size_t)(n_max + 2) * sizeof(int)));
    }
    ~Gabriel_computer()
    {
        ya_free(d_dense);
        if (d_workspace) ya_free(d_workspace);
    }
    Gabriel_computer(const Gabriel_computer&) = delete;
    static constexpr bool carries = false;  // (d_X pipeline only: Heun_solver::take_steps is the loop)

protected:
    int* d_dense = nullptr;  // [0] cells left to gabriel_force_dense, [1] their largest count, then the cells
    float* d_workspace = nullptr;
    size_t workspace_floats = 0;
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints(const int n, const Pt* __restrict__ d_X, const float3* __restrict__ d_old_v,
        Pt* d_dX, const bool has_gen, const int n_active, const bool keep_sorted)
    {
        assert(n_active == n);
        this->grid.build_sorted(n, d_X, d_old_v, this->cube_size, this->d_sorted, this->d_sorted_v);
        if (this->force_variant == 0) {
#ifdef YA_EXPERIMENTAL_FORCE_VARIANTS
            ya::gabriel_force_direct<Pt, pw_int, pw_friction><<<(n + 63) / 64, 64>>>(n, this->d_sorted,
                this->d_sorted_v, this->grid.d_cube_id, this->grid.offsets(), this->grid.grid_size,
                this->grid.n_cubes, this->cube_size, gabriel_coefficient, d_dX, has_gen);
            return;
#else
            fprintf(stderr, "yalla-hip: Gabriel_computer::force_variant 0 is an A/B baseline kept in "
                            "tools/ab/force_variants.cuh: compile with -DYA_EXPERIMENTAL_FORCE_VARIANTS -Itools/ab\n");
            abort();
#endif
        }
        YA_CHECK(ya_memset_async(d_dense, 0, 2 * sizeof(int), nullptr));
        ya::gabriel_force<Pt, pw_int, pw_friction><<<(n + ya::GABRIEL_CELLS - 1) / ya::GABRIEL_CELLS, 64>>>(n,
            this->d_sorted, this->d_sorted_v, this->grid.d_cube_id, this->grid.offsets(), this->grid.grid_size,
            this->grid.n_cubes, this->cube_size, gabriel_coefficient, d_dX, has_gen, d_dense + 2, d_dense);
        // the step waits for the count here (this solver has no captured or overlapped step to protect)
        int h_dense[2];
        YA_CHECK(ya_memcpy_d2h(h_dense, d_dense, sizeof(h_dense)));
        if (h_dense[0] == 0) return;
        // one wavefront per dense cell, each with lists of the largest count, within ~256 MiB if it can be
        const long stride = h_dense[1];
        const size_t per_block = ya::GABRIEL_DENSE_ARRAYS * (size_t)stride;
        int blocks = (int)std::min<size_t>((size_t)h_dense[0], std::max<size_t>(1, (64u << 20) / per_block));
        blocks = std::min(blocks, 2048);
        if (per_block * blocks > workspace_floats) {
            if (d_workspace) ya_free(d_workspace);
            workspace_floats = per_block * blocks;
            YA_CHECK(ya_malloc((void**)&d_workspace, workspace_floats * sizeof(float)));
        }
        ya::gabriel_force_dense<Pt, pw_int, pw_friction><<<blocks, 64>>>(d_dense + 2, d_dense, this->d_sorted,
            this->d_sorted_v, this->grid.d_cube_id, this->grid.offsets(), this->grid.grid_size,
            this->grid.n_cubes, this->cube_size, gabriel_coefficient, d_dX, has_gen, d_workspace, stride);
    }
};

template<typename Pt>
using Gabriel_solver = Heun_solver<Pt, Gabriel_computer>;
