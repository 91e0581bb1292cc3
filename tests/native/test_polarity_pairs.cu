// The polarity force library (include/polarity.cuh) INSIDE the solvers' force kernels, with the kernel's own
// `dist`: tests/polarity_cases.py writes isolated pairs of Po_cells (one partner per cell within the cut-off, so a
// cell's force is one pair term), this program steps them once per library function through every force kernel
// family and writes what the functor was handed and what it returned; tests/test_polarity_pairs_gpu.py holds the
// records to the float64 statement (tests/polarity_statement.py).  Built twice (tests/native/Makefile): the exact
// tier, and test_polarity_pairs_fast with -DYA_ARITH_FAST -ffp-contract=fast.
//
//   test_polarity_pairs <cases> <records>
//
// <cases>:   12 floats per case -- Xi[5], Xj[5], function tag, pref_angle; cell 2c is Xi, cell 2c + 1 is Xj.
// <records>: per recording solver (Tile, Grid default, Grid force_variant 0, Grid force_variant 1, Gabriel), per
//            cell, 6 floats: dist and the Po_cell its function returned.
// stdout:    how often ya::dist3 returns less than |z| on and beside the polar axis, the cells that differ between the several-lanes kernels
//            (functor declared YA_STATELESS) and the one-lane kernels after a step with dt = 0.05.
#include "../../include/dtypes.cuh"
#include "../../include/polarity.cuh"
#include "../../include/solvers.cuh"

#include <cstdio>
#include <cstring>
#include <vector>

static const char* const TIER =
#ifdef YA_ARITH_FAST
    "fast";
#else
    "exact";
#endif
constexpr int GRID_SIZE = 128;  // tests/polarity_cases.py: sites within +-60, Xi at most 1 further

__device__ float* d_records;         // 6 per cell
__device__ int* d_recorded;          // per cell: its record is written
__device__ const float* d_pref;      // per cell

// The library function TAG (tests/polarity_statement.py's order) as a model's functor would call it; the two
// polarization forces take the partner's polarity as bending_force recovers it, Xi - r.
template<int TAG>
__device__ Po_cell library(Po_cell Xi, Po_cell r, float dist, int i)
{
    if (TAG == 0) return unidirectional_polarization_force(Xi, Polarity{Xi.theta - r.theta, Xi.phi - r.phi});
    if (TAG == 1) return bidirectional_polarization_force(Xi, Polarity{Xi.theta - r.theta, Xi.phi - r.phi});
    if (TAG == 2) return bending_force(Xi, r, dist);
    if (TAG == 3) return apical_constriction_force(Xi, r, dist, d_pref[i]);
    return migration_force(Xi, r, dist);
}

// What goes on into the step: a NaN component (the 0 / 0 of migration_force) as 0, or the fixed centre of mass
// would hand it to every other cell's second stage.  The record keeps the NaN.
__device__ Po_cell finite_part(Po_cell F)
{
    float* f = reinterpret_cast<float*>(&F);
    for (int k = 0; k < 5; k++)
        if (!(fabsf(f[k]) <= 3.4e38f)) f[k] = 0.f;
    return F;
}

// One thread owns cell i for the stage (this functor is not declared stateless), so the flag needs no atomic.
template<int TAG>
__device__ Po_cell recording(Po_cell Xi, Po_cell r, float dist, int i, int j)
{
    Po_cell dF{0};
    if (i == j || dist >= 1.f) return dF;
    dF = library<TAG>(Xi, r, dist, i);
    if (!d_recorded[i]) {
        d_recorded[i] = 1;
        float* out = d_records + 6 * (size_t)i;
        out[0] = dist;
        out[1] = dF.x, out[2] = dF.y, out[3] = dF.z, out[4] = dF.theta, out[5] = dF.phi;
    }
    return finite_part(dF);
}

// The twins without stores: `declared` goes to the several-lanes kernels, `plain` stays on one lane per cell.
template<int TAG>
__device__ Po_cell plain(Po_cell Xi, Po_cell r, float dist, int i, int j)
{
    Po_cell dF{0};
    if (i == j || dist >= 1.f) return dF;
    return finite_part(library<TAG>(Xi, r, dist, i));
}
template<int TAG>
__device__ Po_cell declared(Po_cell Xi, Po_cell r, float dist, int i, int j)
{
    Po_cell dF{0};
    if (i == j || dist >= 1.f) return dF;
    return finite_part(library<TAG>(Xi, r, dist, i));
}
YA_STATELESS(Po_cell, declared<0>)
YA_STATELESS(Po_cell, declared<1>)
YA_STATELESS(Po_cell, declared<2>)
YA_STATELESS(Po_cell, declared<3>)
YA_STATELESS(Po_cell, declared<4>)

// How often the pair distance of an axis pair comes out BELOW |r.z| (then r.z / dist > 1 and acosf is NaN): every
// binary32 z in [2^-6, 2^6), r = (0, 0, z) and r = (2^-13 z, 0, z), whose x^2 is a quarter ulp of z^2 at most; and
// the share of both counts that falls on z in [0.5, 1), where the cases' own axis pairs lie.
__global__ void count_undershoot(unsigned first, unsigned last, unsigned long long* counts)
{
    unsigned long long axis = 0, offset = 0, above = 0, axis_cases = 0, offset_cases = 0;
    for (unsigned long long u = (unsigned long long)first + blockIdx.x * blockDim.x + threadIdx.x; u < last;
         u += (unsigned long long)gridDim.x * blockDim.x) {
        const float z = __int_as_float((int)(unsigned)u);
        const bool on_axis = ya::dist3(0.f, 0.f, z) < z, beside = ya::dist3(0x1p-13f * z, 0.f, z) < z;
        axis += on_axis;
        offset += beside;
        above += ya::dist3(0.f, 0.f, z) > z;
        axis_cases += on_axis && z >= 0.5f && z < 1.f;
        offset_cases += beside && z >= 0.5f && z < 1.f;
    }
    if (axis) atomicAdd(counts, axis);
    if (offset) atomicAdd(counts + 1, offset);
    if (above) atomicAdd(counts + 2, above);
    if (axis_cases) atomicAdd(counts + 3, axis_cases);
    if (offset_cases) atomicAdd(counts + 4, offset_cases);
}

static std::vector<Po_cell> cells;
static std::vector<float> prefs;
static std::vector<int> tags;
static float* records_dev;
static int* recorded_dev;

template<typename Solution_t>
static void load(Solution_t& s)
{
    const int n = (int)cells.size();
    *s.h_n = n;
    memcpy(s.h_X, cells.data(), n * sizeof(Po_cell));
    s.copy_to_device();
}

// One step with dt = 0 under the recording functor of TAG; the records of the cells tagged TAG go to `merged`.
template<int TAG, typename Solution_t>
static void record_one(Solution_t& s, std::vector<float>& merged)
{
    const int n = (int)cells.size();
    load(s);
    YA_CHECK((int)hipMemset(recorded_dev, 0, n * sizeof(int)));
    YA_CHECK((int)hipMemset(records_dev, 0xff, 6 * n * sizeof(float)));  // (a cell never called stays NaN)
    s.template take_step<recording<TAG>, friction_on_background<Po_cell>>(0.f);
    YA_CHECK((int)hipDeviceSynchronize());
    std::vector<float> got(6 * (size_t)n);
    YA_CHECK(ya_memcpy_d2h(got.data(), records_dev, got.size() * sizeof(float)));
    for (int i = 0; i < n; i++)
        if (tags[i] == TAG) memcpy(&merged[6 * (size_t)i], &got[6 * (size_t)i], 6 * sizeof(float));
}

// `with_fresh` hands a newly made Solution to its argument, one per function: no state carries over.
template<typename Make>
static void record_all(const char* name, FILE* out, Make with_fresh)
{
    std::vector<float> merged(6 * cells.size());
    with_fresh([&](auto& s) { record_one<0>(s, merged); });
    with_fresh([&](auto& s) { record_one<1>(s, merged); });
    with_fresh([&](auto& s) { record_one<2>(s, merged); });
    with_fresh([&](auto& s) { record_one<3>(s, merged); });
    with_fresh([&](auto& s) { record_one<4>(s, merged); });
    fwrite(merged.data(), sizeof(float), merged.size(), out);
    printf("recorded %s\n", name);
}

template<Pairwise_interaction<Po_cell> force, typename Solution_t>
static std::vector<Po_cell> stepped(Solution_t& s)
{
    load(s);
    s.template take_step<force, friction_on_background<Po_cell>>(0.05f);
    s.copy_to_host();
    return std::vector<Po_cell>(s.h_X, s.h_X + cells.size());
}

static int differing(const std::vector<Po_cell>& a, const std::vector<Po_cell>& b)
{
    int different = 0;
    for (size_t i = 0; i < a.size(); i++) different += memcmp(&a[i], &b[i], sizeof(Po_cell)) != 0;
    return different;
}

// A step with dt = 0.05 from the cases' state: the several-lanes kernels (functor declared stateless) against the
// one-lane kernels (its undeclared twin), bit for bit.
template<int TAG>
static int twins()
{
    const int n = (int)cells.size();
    int different = 0;
    std::vector<Po_cell> one_lane;
    {
        Solution<Po_cell, Tile_solver> s{n};
        s.lanes_per_cell = 1;
        one_lane = stepped<plain<TAG>>(s);
    }
    for (int lanes : {0, 16, 64}) {  // 0: the solver's own choice for a declared functor
        Solution<Po_cell, Tile_solver> s{n};
        s.lanes_per_cell = lanes;
        different += differing(one_lane, stepped<declared<TAG>>(s));
    }
    {
        Solution<Po_cell, Grid_solver> s{n, GRID_SIZE, 1.f};
        one_lane = stepped<plain<TAG>>(s);
    }
    for (int lanes : {0, 4, 8, 16}) {
        Solution<Po_cell, Grid_solver> s{n, GRID_SIZE, 1.f};
        s.force_variant = 3;
        s.coop_lanes = lanes;
        different += differing(one_lane, stepped<declared<TAG>>(s));
    }
    return different;
}

int main(int argc, char** argv)
{
    static_assert(!ya::stateless_pair<Po_cell, recording<2>, friction_on_background<Po_cell>>(), "");
    static_assert(!ya::stateless_pair<Po_cell, plain<2>, friction_on_background<Po_cell>>(), "");
    static_assert(ya::stateless_pair<Po_cell, declared<2>, friction_on_background<Po_cell>>(), "");
    if (argc != 3) return fprintf(stderr, "usage: %s <cases> <records>\n", argv[0]), 2;
    {
        FILE* in = fopen(argv[1], "rb");
        if (!in) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
        float c[12];
        while (fread(c, sizeof(float), 12, in) == 12) {
            cells.push_back(Po_cell{c[0], c[1], c[2], c[3], c[4]});
            cells.push_back(Po_cell{c[5], c[6], c[7], c[8], c[9]});
            for (int k = 0; k < 2; k++) tags.push_back((int)c[10]), prefs.push_back(c[11]);
        }
        fclose(in);
    }
    const int n = (int)cells.size();
    printf("tier %s, %d cells\n", TIER, n);
    if (n == 0) return 2;

    {  // the measurement first
        unsigned long long *d_counts, counts[5];
        YA_CHECK(ya_malloc((void**)&d_counts, sizeof(counts)));
        YA_CHECK((int)hipMemset(d_counts, 0, sizeof(counts)));
        const unsigned first = 0x3C800000u, last = 0x42800000u;  // 2^-6, 2^6
        count_undershoot<<<4096, 256>>>(first, last, d_counts);
        YA_CHECK(ya_memcpy_d2h(counts, d_counts, sizeof(counts)));
        ya_free(d_counts);
        printf("dist3 below z: axis %llu offset %llu of %u (above z on the axis: %llu; z in [0.5, 1): axis %llu offset "
               "%llu)\n", counts[0], counts[1], last - first, counts[2], counts[3], counts[4]);
    }

    float* pref_dev;
    YA_CHECK(ya_malloc((void**)&records_dev, 6 * (size_t)n * sizeof(float)));
    YA_CHECK(ya_malloc((void**)&recorded_dev, n * sizeof(int)));
    YA_CHECK(ya_malloc((void**)&pref_dev, n * sizeof(float)));
    YA_CHECK(ya_memcpy_h2d(pref_dev, prefs.data(), n * sizeof(float)));
    YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(d_records), &records_dev, sizeof(float*)));
    YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(d_recorded), &recorded_dev, sizeof(int*)));
    YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(d_pref), &pref_dev, sizeof(float*)));

    FILE* out = fopen(argv[2], "wb");
    if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    record_all("Tile_solver", out, [&](auto run) {
        Solution<Po_cell, Tile_solver> s{n};
        run(s);
    });
    for (int variant : {-1, 0, 1})
        record_all(variant < 0 ? "Grid_solver" : variant ? "Grid_solver force_variant 1" : "Grid_solver force_variant 0",
            out, [&](auto run) {
                Solution<Po_cell, Grid_solver> s{n, GRID_SIZE, 1.f};
                s.force_variant = variant;
                run(s);
            });
    record_all("Gabriel_solver", out, [&](auto run) {
        Solution<Po_cell, Gabriel_solver> s{n, GRID_SIZE, 1.f};
        run(s);
    });
    fclose(out);

    const int different = twins<0>() + twins<1>() + twins<2>() + twins<3>() + twins<4>();
    printf("several-lanes kernels against one lane: %d cells differ\n", different);

    ya_free(records_dev);
    ya_free(recorded_dev);
    ya_free(pref_dev);
    if (different == 0) printf("ALL POLARITY PAIR RUNS DONE\n");
    return different != 0;
}
