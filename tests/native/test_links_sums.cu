// Links::link_forces at force level, both device implementations: the one-thread-per-link kernel with its atomics
// (links_segmented_min() = 1 << 30) and the segmented sum (links_segmented_min() = 1).
//
// EXACT INPUTS.  Cells on an integer lattice, every link along one axis, strength 0.25: r = (+-k, 0, 0), dist = k,
// every term +-0.25 or 0, every partial sum a small multiple of 0.25 -- the answer does not depend on the order of
// the additions, so one integer count per cell and axis, times 0.25f, holds both paths, any number of pieces, plain
// and atomic stores, with memcmp.  Sizes around the launch's block edge, hub segments of 255 .. 513 entries placed
// at chosen offsets of the sorted entry array (on, before and behind the cut every 256 entries), inert links, every
// way of setting *d_n, float4 and Po_cell points, the scratch buffers from call to call, a custom Link_force.
//
// GENERAL INPUTS.  Random binary32 positions, ids unrelated to slot order: the segmented path against a host
// restatement of the header's comment (entries 2i / 2i + 1, stable sort by cell, a cut at every multiple of 256,
// each piece summed from 0.f in sorted order) bit for bit wherever the order of the additions is fixed, and both
// paths against a binary64 evaluation within a derived bound (at `bound`).
#include "../../include/dtypes.cuh"
#include "../../include/links.cuh"
#include "../../include/solvers.cuh"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            failures++;                                               \
        }                                                             \
    } while (0)

enum Path { SEGMENTED = 0, ATOMICS = 1 };
static const char* path_name[] = {"segmented", "atomics"};

__global__ void set_count(int* d_n, int value)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_n = value;
}

// A custom Link_force: a spring without rest length, dX[a] -= s r, dX[b] += s r.  On the lattice s r is a multiple
// of 0.25.
template<typename Pt>
__device__ void hooke_force(const Pt* __restrict__ d_X, const int a, const int b, const float strength, Pt* d_dX)
{
    const Pt r = d_X[a] - d_X[b];
    atomicAdd(&d_dX[a].x, -strength * r.x);
    atomicAdd(&d_dX[a].y, -strength * r.y);
    atomicAdd(&d_dX[a].z, -strength * r.z);
    atomicAdd(&d_dX[b].x, strength * r.x);
    atomicAdd(&d_dX[b].y, strength * r.y);
    atomicAdd(&d_dX[b].z, strength * r.z);
}

template<typename Pt>
constexpr int n_floats()
{
    return (int)(sizeof(Pt) / sizeof(float));
}

// X and dX0 (n cells of Pt, as floats) to the device, link_forces on `path`, dX back.  lower_to >= 0: a one-thread
// kernel writes that count to *d_n immediately before the call.  custom: link_forces<Pt, hooke_force<Pt>>.
template<typename Pt>
std::vector<float> forces(Links& links, const std::vector<float>& X, const std::vector<float>& dX0, Path path,
    int lower_to = -1, bool custom = false)
{
    const size_t bytes = X.size() * sizeof(float);
    Pt *d_X, *d_dX;
    std::vector<float> out(dX0.size(), -99.f);
    EXPECT(X.size() == dX0.size() && X.size() % n_floats<Pt>() == 0);
    EXPECT(hipMalloc(&d_X, bytes) == hipSuccess);
    EXPECT(hipMalloc(&d_dX, bytes) == hipSuccess);
    EXPECT(hipMemcpy(d_X, X.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
    EXPECT(hipMemcpy(d_dX, dX0.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
    ya::links_segmented_min() = path == SEGMENTED ? 1 : (1 << 30);
    if (lower_to >= 0) set_count<<<1, 1>>>(links.d_n, lower_to);
    if (custom) link_forces<Pt, hooke_force<Pt>>(links, d_X, d_dX);
    else link_forces<Pt>(links, d_X, d_dX);
    EXPECT(hipDeviceSynchronize() == hipSuccess);
    EXPECT(hipMemcpy(out.data(), d_dX, bytes, hipMemcpyDeviceToHost) == hipSuccess);
    (void)hipFree(d_X);
    (void)hipFree(d_dX);
    return out;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static void report(const char* what, Path path, const std::vector<float>& got, const std::vector<float>& want, int nf)
{
    if (same_bits(got, want)) return;
    for (size_t k = 0; k < got.size(); k++)
        if (memcmp(&got[k], &want[k], sizeof(float)) != 0) {
            printf("FAIL %s (%s): cell %zu component %zu: got %.9g, expected %.9g\n", what, path_name[path], k / nf,
                k % nf, got[k], want[k]);
            break;
        }
    failures++;
}

// ---- the lattice ----------------------------------------------------------------------------------------------------
// Cell c sits on arm c % 3 (the x, y or z axis through P) at P + off(c) e_arm, off(c) = +-(c / 3 + 1) by the parity
// of c / 3; the hub sits on P itself.  A link is legal between two cells of one arm, or between the hub and any
// cell: exactly one component of r is a non-zero integer, |k| <= 2 (n / 3 + 1) <= 1000.
struct Lattice {
    int n, hub;
    std::vector<int> at;  // 3 n integer coordinates
    Lattice(int n, int hub) : n{n}, hub{hub}, at(3 * n)
    {
        const int P[3] = {5, -3, 2};
        EXPECT(2 * (n / 3 + 1) <= 1000);
        for (int c = 0; c < n; c++) {
            for (int k = 0; k < 3; k++) at[3 * c + k] = P[k];
            if (c == hub) continue;
            const int off = (c / 3 + 1) * ((c / 3) % 2 ? -1 : 1);
            at[3 * c + c % 3] += off;
        }
    }
    template<typename Pt>
    std::vector<float> positions() const
    {
        const int nf = n_floats<Pt>();
        std::vector<float> X((size_t)n * nf);
        for (int c = 0; c < n; c++)
            for (int k = 0; k < nf; k++) X[(size_t)c * nf + k] = k < 3 ? (float)at[3 * c + k] : 0.125f * (c % 7) - k;
        return X;
    }
    // Starting dX: multiples of 0.25, 3.5 or -1.25 for two cells in three, the further components sentinels.
    template<typename Pt>
    std::vector<float> start() const
    {
        const int nf = n_floats<Pt>();
        std::vector<float> dX((size_t)n * nf);
        for (int c = 0; c < n; c++)
            for (int k = 0; k < nf; k++)
                dX[(size_t)c * nf + k] = k < 3 ? (c % 3 == 0 ? 3.5f : c % 3 == 1 ? 0.f : -1.25f - k) : 1000.f + 10 * c + k;
        return dX;
    }
    // Integer arithmetic: the first n_live slots, a == b skipped; the term is the sign of the one non-zero
    // component of r (hooke: the component itself), -term on a and +term on b, then times 0.25f.
    template<typename Pt>
    std::vector<float> expected(const std::vector<Link>& links, int n_live, bool hooke = false) const
    {
        const int nf = n_floats<Pt>();
        std::vector<long> count(3 * n, 0);
        for (int i = 0; i < n_live; i++) {
            const int a = links[i].a, b = links[i].b;
            if (a == b) continue;
            int axes = 0;
            for (int k = 0; k < 3; k++) {
                const int r = at[3 * a + k] - at[3 * b + k];
                if (r == 0) continue;
                axes++;
                EXPECT(abs(r) <= 1000);
                const int term = hooke ? r : (r > 0 ? 1 : -1);
                count[3 * a + k] -= term;
                count[3 * b + k] += term;
            }
            EXPECT(axes == 1);
        }
        std::vector<float> want = start<Pt>();
        for (int c = 0; c < n; c++)
            for (int k = 0; k < 3; k++) {
                EXPECT(labs(count[3 * c + k]) < (1 << 20));
                want[(size_t)c * nf + k] += 0.25f * (float)count[3 * c + k];
            }
        return want;
    }
};

static void fill(Links& links, const std::vector<Link>& l, int n_live)
{
    EXPECT((int)l.size() == links.n_max && n_live <= links.n_max);
    for (int i = 0; i < links.n_max; i++) links.h_link[i] = l[i];
    *links.h_n = n_live;
    links.copy_to_device();
}

// Both paths on the links `l` (all of them slots of one Links, the first n_live in use).
template<typename Pt>
void both_paths(const char* what, const Lattice& lat, const std::vector<Link>& l, int n_live)
{
    Links links{(int)l.size(), 0.25f};
    fill(links, l, n_live);
    const auto want = lat.expected<Pt>(l, n_live);
    for (Path path : {SEGMENTED, ATOMICS})
        report(what, path, forces<Pt>(links, lat.positions<Pt>(), lat.start<Pt>(), path), want, n_floats<Pt>());
}

// ---- sizes: n_max around the launch's block edge, every slot in use ---------------------------------------------
static void sizes()
{
    const Lattice lat{900, 450};
    for (int n_max : {1, 127, 128, 129, 255, 256, 257}) {
        std::vector<Link> l;
        for (int i = 0; i < n_max; i++) {
            // along the arms, either way round, every cell in two links; the hub in every 9th
            const int c = i % 440;
            Link link = i % 2 ? Link{c + 3, c} : Link{c, c + 3};
            if (i % 9 == 4) link = Link{lat.hub, c};
            l.push_back(link);
        }
        char what[64];
        snprintf(what, sizeof what, "n_max = %d", n_max);
        both_paths<float3>(what, lat, l, n_max);
    }
}

// ---- a hub segment of `length` entries that starts at `offset` in the sorted entry array -------------------------
// offset / 2 filler links between cells below the hub put two entries each in front of it, offset % 2 links from
// below the hub to above it one; then `length` links hub -- partner (ids above the hub's, the hub as a or b), a tail
// of links between cells above the hub, and an inert link every 17 slots, all interleaved.
static std::vector<Link> hub_links(const Lattice& lat, int offset, int length)
{
    const int hub = lat.hub;
    std::vector<Link> fillers, hubs, tail, l;
    EXPECT(offset / 2 + 4 < hub && hub + length + 40 < lat.n);
    for (int k = 0; k < offset / 2; k++) {
        const int c = (5 * k) % (hub - 3);  // (c, c + 3): one arm, both below the hub
        fillers.push_back(k % 2 ? Link{c, c + 3} : Link{c + 3, c});
    }
    if (offset % 2) fillers.push_back(Link{hub + 6, hub - 3});  // (one arm: the ids differ by 9)
    for (int k = 0; k < length; k++) hubs.push_back(k % 3 == 1 ? Link{hub + 1 + k, hub} : Link{hub, hub + 1 + k});
    for (int k = 0; k < 31; k++) tail.push_back(Link{hub + 1 + k + 3, hub + 1 + k});
    size_t f = 0, h = 0, t = 0;
    while (f < fillers.size() || h < hubs.size() || t < tail.size()) {
        if (l.size() % 17 == 5) l.push_back(Link{(int)l.size() % lat.n, (int)l.size() % lat.n});  // inert
        if (h < hubs.size()) l.push_back(hubs[h++]);
        if (f < fillers.size()) l.push_back(fillers[f++]);
        if (h < hubs.size()) l.push_back(hubs[h++]);
        if (t < tail.size()) l.push_back(tail[t++]);
    }
    // what the layout is for: the number of entries in front of the hub's, and the hub's own
    int before = 0, own = 0;
    for (const Link& k : l) {
        if (k.a == k.b) continue;
        before += (k.a < hub) + (k.b < hub);
        own += (k.a == hub) + (k.b == hub);
    }
    EXPECT(before == offset && own == length);
    return l;
}

template<typename Pt>
void hubs()
{
    const Lattice lat{1200, 400};
    for (int length : {255, 256, 257, 512, 513}) {
        // offsets modulo 256: 0 (length 256: the segment fills one window and is not cut), 1, 255 (a head piece of
        // one entry), the offset at which the last piece has one entry, and 0 again one window further on
        for (int offset : {0, 1, 255, (256 + 1 - length % 256) % 256, 256}) {
            char what[64];
            snprintf(what, sizeof what, "hub of %d entries at offset %d, %d floats", length, offset, n_floats<Pt>());
            const auto l = hub_links(lat, offset, length);
            both_paths<Pt>(what, lat, l, (int)l.size());
        }
    }
}

// ---- *d_n ---------------------------------------------------------------------------------------------------------
static void counts()
{
    const Lattice lat{1200, 400};
    auto l = hub_links(lat, 7, 300);  // every slot a live-looking link, or inert
    const int n_max = (int)l.size();
    Links links{n_max, 0.25f};
    const auto X = lat.positions<float3>(), dX0 = lat.start<float3>();
    for (Path path : {SEGMENTED, ATOMICS}) {
        for (int n_live : {0, 1, n_max - 1, n_max, n_max / 2}) {
            fill(links, l, n_max);
            links.set_d_n(n_live);
            EXPECT(links.get_d_n() == n_live);
            report("*d_n through set_d_n", path, forces<float3>(links, X, dX0, path), lat.expected<float3>(l, n_live), 3);
        }
        // lowered on the device right before the call, as a model kernel may
        for (int n_live : {0, 1, 257, n_max - 1}) {
            fill(links, l, n_max);
            report("*d_n lowered by a kernel", path, forces<float3>(links, X, dX0, path, n_live),
                lat.expected<float3>(l, n_live), 3);
            EXPECT(links.get_d_n() == n_live);
        }
    }
}

// ---- the scratch buffers from call to call -----------------------------------------------------------------------
static void scratch()
{
    const Lattice lat{1200, 400};
    const auto first = hub_links(lat, 255, 513), other = hub_links(lat, 1, 257);
    auto fewer = first;  // the same slots with fewer live links: two in three inert now, and a lower count
    for (size_t i = 0; i < fewer.size(); i++)
        if (i % 3) fewer[i] = Link{(int)i % 50, (int)i % 50};
    const int fewer_live = (int)fewer.size() - 200;
    const auto X = lat.positions<float3>(), dX0 = lat.start<float3>();
    for (Path path : {SEGMENTED, ATOMICS}) {
        Links a{(int)first.size(), 0.25f}, b{(int)other.size(), 0.25f};
        fill(a, first, (int)first.size());
        fill(b, other, (int)other.size());
        report("first call", path, forces<float3>(a, X, dX0, path), lat.expected<float3>(first, (int)first.size()), 3);
        report("another Links", path, forces<float3>(b, X, dX0, path), lat.expected<float3>(other, (int)other.size()), 3);
        fill(a, fewer, fewer_live);
        report("fewer live links", path, forces<float3>(a, X, dX0, path), lat.expected<float3>(fewer, fewer_live), 3);
        report("another Links again", path, forces<float3>(b, X, dX0, path),
            lat.expected<float3>(other, (int)other.size()), 3);
        report("fewer live links again", path, forces<float3>(a, X, dX0, path), lat.expected<float3>(fewer, fewer_live), 3);
        fill(a, first, (int)first.size());
        report("all of them back", path, forces<float3>(a, X, dX0, path),
            lat.expected<float3>(first, (int)first.size()), 3);
    }
}

// ---- a custom Link_force keeps the one-thread-per-link kernel, whatever the threshold says ---------------------
template<typename Pt>
void custom()
{
    const Lattice lat{1200, 400};
    const auto l = hub_links(lat, 3, 300);
    const int n_live = (int)l.size() - 5;
    Links links{(int)l.size(), 0.25f};
    fill(links, l, n_live);
    const auto want = lat.expected<Pt>(l, n_live, true);
    EXPECT(!same_bits(want, lat.expected<Pt>(l, n_live)));  // (not what the default force gives)
    for (Path path : {SEGMENTED, ATOMICS})
        report("custom force", path, forces<Pt>(links, lat.positions<Pt>(), lat.start<Pt>(), path, -1, true), want,
            n_floats<Pt>());
}

// ---- general inputs ----------------------------------------------------------------------------------------------
static uint32_t lcg_state = 12345u;
static uint32_t lcg()
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}

static void general()
{
    const int n = 1500, n_max = 2600, n_live = 2500, hub = 700;
    const float strength = 0.2f;
    std::vector<float> X(3 * n), dX0(3 * n);
    for (int c = 0; c < n; c++)
        for (int k = 0; k < 3; k++) {
            X[3 * c + k] = (float)(lcg() % 100000) * 1e-4f - 5.f;
            dX0[3 * c + k] = c % 2 ? (float)(lcg() % 1000) * 1e-3f - 0.5f : 0.f;  // even ids start from zero
        }
    std::vector<Link> l(n_max);
    for (int i = 0; i < n_max; i++) {
        // (ids 1400 .. 1499 in no link at all: they must keep their bits)
        l[i] = Link{(int)(lcg() % 1400), (int)(lcg() % 1400)};
        if (i % 37 == 11) l[i].b = l[i].a;                                  // inert
        if (i >= 900 && i < 1600) (i % 2 ? l[i].a : l[i].b) = hub;          // a hub of ~700 entries: three pieces or four
    }
    Links links{n_max, strength};
    fill(links, l, n_live);

    // The statement of links.cuh's comment in binary32 on the host: f of every link, entries 2i (cell a, -f) and
    // 2i + 1 (cell b, +f), a stable sort by cell with dead slots last, a cut at every multiple of 256 of the sorted
    // array, each piece summed from 0.f in sorted order.
    std::vector<float> f(3 * n_max, 0.f);
    std::vector<uint32_t> key(2 * n_max, 0xFFFFFFFFu), entry(2 * n_max);
    for (int i = 0; i < n_max; i++) {
        entry[2 * i] = 2 * i;
        entry[2 * i + 1] = 2 * i + 1;
        if (i >= n_live || l[i].a == l[i].b) continue;
        float r[3];
        for (int k = 0; k < 3; k++) r[k] = X[3 * l[i].a + k] - X[3 * l[i].b + k];
        const float dist = sqrtf(fmaf(r[2], r[2], fmaf(r[1], r[1], r[0] * r[0])));
        for (int k = 0; k < 3; k++) f[3 * i + k] = strength * r[k] / dist;
        key[2 * i] = (uint32_t)l[i].a;
        key[2 * i + 1] = (uint32_t)l[i].b;
    }
    std::stable_sort(entry.begin(), entry.end(), [&](uint32_t p, uint32_t q) { return key[p] < key[q]; });
    std::vector<int> pieces(n, 0), terms(n, 0);
    std::vector<float> piece_sum(3 * n * 2, 0.f);  // the first two pieces of every cell
    std::vector<double> want64(3 * n, 0.), abs64(3 * n, 0.);
    for (size_t t = 0; t < entry.size();) {
        const uint32_t cell = key[entry[t]];
        if (cell == 0xFFFFFFFFu) break;
        float s[3] = {0.f, 0.f, 0.f};
        size_t u = t;
        do {
            const float sign = entry[u] & 1u ? 1.f : -1.f;
            for (int k = 0; k < 3; k++) s[k] += sign * f[3 * (entry[u] >> 1) + k];
            terms[cell]++;
            u++;
        } while (u < entry.size() && key[entry[u]] == cell && u % 256 != 0);
        if (pieces[cell] < 2)
            for (int k = 0; k < 3; k++) piece_sum[(3 * cell + k) * 2 + pieces[cell]] = s[k];
        pieces[cell]++;
        t = u;
    }
    // ... and the same forces in binary64 from the same binary32 positions
    for (int i = 0; i < n_live; i++) {
        if (l[i].a == l[i].b) continue;
        double r[3];
        for (int k = 0; k < 3; k++) r[k] = (double)X[3 * l[i].a + k] - (double)X[3 * l[i].b + k];
        const double dist = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        for (int k = 0; k < 3; k++) {
            const double term = (double)strength * r[k] / dist;
            want64[3 * l[i].a + k] -= term;
            want64[3 * l[i].b + k] += term;
            abs64[3 * l[i].a + k] += std::fabs(term);
            abs64[3 * l[i].b + k] += std::fabs(term);
        }
    }
    // The bound for a sum whose order is not fixed, u = 2^-24 (half an ulp, relative), m terms on a start value d:
    //   - a term: the components of r are rounded differences (1 u each: 1 u on r.c and at most 1 u on |r|); x x,
    //     fma(y, y, .) and fma(z, z, .) round a sum of non-negative numbers three times (3 u, halved by the square
    //     root: 1.5 u); the square root, the product strength r.c and the quotient round once each (3 u): 6.5 u of
    //     the term to first order, taken as 7 u;
    //   - the additions: m of them in any grouping (a piece's first addition, to 0.f, is exact, and adding a piece
    //     to the cell's value replaces it; with d == 0 one more is exact: m - 1), each rounds a partial sum that is
    //     at most |d| + sum |term| in magnitude: m u (|d| + sum |term|);
    //   - the binary64 evaluation itself and the second-order terms: far below the last 1 u of
    //   |got - want| <= (m + 8) u (|d| + sum |term|),         sum |term| <= m strength.
    // For d == 0 this is the bound (m + 8) 2^-24 sum |term|.
    auto bound = [&](int cell, int k) {
        return (terms[cell] + 8) * std::ldexp(1., -24) * (std::fabs((double)dX0[3 * cell + k]) + abs64[3 * cell + k]);
    };
    int n_one = 0, n_two = 0, n_more = 0, n_untouched = 0, worst_cell = -1;
    double worst = 0;
    std::vector<float> runs[2];
    for (int run = 0; run < 2; run++) runs[run] = forces<float3>(links, X, dX0, SEGMENTED);
    const auto atomics = forces<float3>(links, X, dX0, ATOMICS);
    for (int cell = 0; cell < n; cell++) {
        EXPECT(terms[cell] * (double)strength >= abs64[3 * cell] - 1e-9);
        for (int k = 0; k < 3; k++) {
            const int at = 3 * cell + k;
            const float got = runs[0][at];
            const float p0 = piece_sum[at * 2], p1 = piece_sum[at * 2 + 1];
            bool ok = true, fixed_order = true;
            float want = 0.f;
            if (pieces[cell] == 0) want = dX0[at];                          // no link: the bits it had
            else if (pieces[cell] == 1) want = dX0[at] + p0;                // a plain store of dX0 + piece
            else if (pieces[cell] == 2 && dX0[at] == 0.f) want = p0 + p1;   // two atomics on zero: they commute
            else fixed_order = false;
            if (fixed_order) {
                ok = memcmp(&got, &want, sizeof(float)) == 0 && memcmp(&got, &runs[1][at], sizeof(float)) == 0;
            } else {
                for (int run = 0; run < 2; run++)
                    ok = ok && std::fabs((double)runs[run][at] - (dX0[at] + want64[at])) <= bound(cell, k);
            }
            if (!ok) {
                printf("FAIL general inputs (segmented): cell %d component %d, %d pieces: got %.9g and %.9g, expected %.9g"
                       " (binary64 %.9g)\n", cell, k, pieces[cell], got, runs[1][at], want, dX0[at] + want64[at]);
                failures++;
            }
            // the atomics: any order
            const double err = std::fabs((double)atomics[at] - (dX0[at] + want64[at]));
            if (pieces[cell] == 0) EXPECT(memcmp(&atomics[at], &dX0[at], sizeof(float)) == 0);
            else if (err > bound(cell, k)) {
                printf("FAIL general inputs (atomics): cell %d component %d, %d terms: |%.9g - %.9g| = %.3g > %.3g\n",
                    cell, k, terms[cell], atomics[at], dX0[at] + want64[at], err, bound(cell, k));
                failures++;
            }
            if (pieces[cell] && err / bound(cell, k) > worst) {
                worst = err / bound(cell, k);
                worst_cell = cell;
            }
        }
        n_untouched += pieces[cell] == 0;
        n_one += pieces[cell] == 1;
        n_two += pieces[cell] == 2 && dX0[3 * cell] == 0.f;
        n_more += pieces[cell] >= 3;
    }
    printf("general inputs: %d cells in one piece, %d in two on a zero start, %d in three or more, %d untouched; "
           "atomics at most %.3f of the bound (cell %d)\n", n_one, n_two, n_more, n_untouched, worst, worst_cell);
    // every kind of cell is there
    EXPECT(n_one > 1000 && n_two >= 1 && n_more >= 1 && n_untouched >= 100 && pieces[hub] >= 3);
}

int main()
{
    sizes();
    hubs<float3>();
    hubs<float4>();
    hubs<Po_cell>();
    counts();
    scratch();
    custom<float3>();
    custom<Po_cell>();
    general();
    ya::links_segmented_min() = YA_LINKS_SEGMENTED_MIN;
    if (failures == 0) printf("ALL LINK SUM TESTS PASSED\n");
    return failures != 0;
}
