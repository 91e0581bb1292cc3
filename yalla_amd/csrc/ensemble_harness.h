// What the ensemble harnesses (ensemble.hip, ensemble_links.hip, ensemble_grid.hip, ensemble_gabriel.hip) share: the generic-force
// policies of their model tables, the interfaces their C handles hold, the overrides that forward to an Ensemble,
// the model table, and the bodies of the C entry points that are the same but for the prefix.  Each .hip writes its
// own table, what its form adds, create's checks, set_param, and its exported functions as one-line forwards.
#pragma once

#include <string>
#include <vector>

namespace ens_harness {

template<typename Pt>
struct No_gen {
    static Generic_forces<Pt> gen(int, int) { return no_gen_forces<Pt>; }
    static void before_steps(int) {}
};

// The generic force of the `push_*` models (models::push: the right-hand side of cell 1 set to (1, 0, 0)) for
// an ensemble: ONE call on the flat arrays pushes cell 1 of every replica, global row r * n_max + 1.
template<typename Pt>
__global__ void push_cell_1_of_every_replica(const int n_replicas, const int n_max, Pt* d_dX)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_replicas) return;
    Pt* row = d_dX + (size_t)r * n_max + 1;
    row->x = 1;
    row->y = 0;
    row->z = 0;
}
template<typename Pt>
struct Push_gen {
    static Generic_forces<Pt> gen(int n_replicas, int n_max)
    {
        return [n_replicas, n_max](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            if (n_max < 2 || n != n_replicas * n_max) return;
            push_cell_1_of_every_replica<Pt><<<(n_replicas + 255) / 256, 256>>>(n_replicas, n_max, d_dX);
        };
    }
    static void before_steps(int) {}
};

// A friction that reads its ids' VALUES (models::ids_friction), for an ensemble: the functors of an ensemble get
// global ids (r * n_max + local), so the ensemble's model hands the friction the local ones (as ensemble.hip's
// oscillator_by_local_id does for a force): the same statements, hence the bits of the lone model in every replica.
// n_max travels in a device variable of the library, set when it changes.
__device__ int friction_rows_per_replica = 1;
template<Pairwise_friction<float3> friction>
__device__ inline float friction_by_local_id(float3 Xi, float3 r, float dist, int i, int j)
{
    return friction(Xi, r, dist, i % friction_rows_per_replica, j % friction_rows_per_replica);
}
struct Local_friction_ids : public No_gen<float3> {
    static void before_steps(int n_max)
    {
        static int rows_set = 1;
        if (rows_set == n_max) return;
        YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(friction_rows_per_replica), &n_max, sizeof(int)));
        rows_set = n_max;
    }
};

// THE INTERFACES.  What every form exposes to its C functions, and what the two all-pairs and the two grid forms
// add.  A grid form's take_steps and a form's own setters are declared by the interface each .hip derives from one
// of these.
struct Replicas {
    virtual ~Replicas() {}
    virtual int n_floats() = 0;
    virtual int n_replicas() = 0;
    virtual int n_max() = 0;
    virtual float* h_X() = 0;
    virtual int* h_n() = 0;
    virtual void copy_to_device() = 0;
    virtual void copy_to_host() = 0;
    virtual int get_d_n(int r) = 0;
    virtual void set_fixed(int mode, int point) = 0;
    virtual float3* d_old_v() = 0;
};
struct Tile_replicas : public Replicas {
    virtual long take_steps(float dt, int n_steps) = 0;  // returns the whole-step launches it made
    virtual void set_lanes(int lanes) = 0;
    virtual void set_whole_steps(int mode) = 0;
    virtual void set_steps_per_launch(int steps) = 0;
    virtual void set_whole_step_lanes(int lanes) = 0;
};
struct Grid_replicas : public Replicas {
    virtual int n_cubes() = 0;
    virtual void set_cube_size(float cube_size) = 0;
    virtual int status(int r, bool clear) = 0;
    virtual const int* d_cube_id() = 0;
    virtual const int* d_point_id() = 0;
    virtual const int* d_offs() = 0;
};

// THE OVERRIDES.  Cells is an Ensemble<Pt, Solver>, Interface is or derives from Replicas, Tile_replicas or
// Grid_replicas; the .hip's Sim derives from one of these three and overrides what is left.
template<typename Cells, typename Interface_>
struct Replicas_of : public Interface_ {
    using Interface = Interface_;
    Cells cells;
    template<typename... Args>
    explicit Replicas_of(Args... args) : cells{args...}
    {
    }
    int n_floats() override { return sizeof(*cells.h_X) / sizeof(float); }
    int n_replicas() override { return cells.n_replicas; }
    int n_max() override { return cells.n_max; }
    float* h_X() override { return reinterpret_cast<float*>(cells.h_X); }
    int* h_n() override { return cells.h_n; }
    void copy_to_device() override { cells.copy_to_device(); }
    void copy_to_host() override { cells.copy_to_host(); }
    int get_d_n(int r) override { return cells.get_d_n(r); }
    void set_fixed(int mode, int point) override
    {
        if (mode == 0) cells.set_fixed();
        if (mode == 1) cells.set_fixed(point);
        if (mode == 2) cells.set_fixed_xy(point);
    }
    float3* d_old_v() override { return cells.d_old_v; }
};
template<typename Cells, typename Interface>
struct Tile_replicas_of : public Replicas_of<Cells, Interface> {
    using Replicas_of<Cells, Interface>::Replicas_of;
    using Replicas_of<Cells, Interface>::cells;
    void set_lanes(int lanes) override { cells.lanes_per_cell = lanes; }
    void set_whole_steps(int mode) override { cells.whole_steps = mode; }
    void set_steps_per_launch(int steps) override { cells.steps_per_launch = steps; }
    void set_whole_step_lanes(int lanes) override { cells.whole_step_lanes = lanes; }
};
template<typename Cells, typename Interface>
struct Grid_replicas_of : public Replicas_of<Cells, Interface> {
    using Replicas_of<Cells, Interface>::Replicas_of;
    using Replicas_of<Cells, Interface>::cells;
    int n_cubes() override { return cells.n_cubes; }
    void set_cube_size(float cube_size) override { cells.cube_size = cube_size; }
    int status(int r, bool clear) override { return cells.status(r, clear); }
    const int* d_cube_id() override { return cells.d_cube_id; }
    const int* d_point_id() override { return cells.d_point_id; }
    const int* d_offs() override { return cells.d_offs; }
};
// The Gabriel form's take_steps: one take_step per step, the policy's generic force in each (the grid form's goes
// through Ensemble<Pt, Grid_solver>::take_steps, which is that loop unless "lds_steps" allows launches from LDS).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy,
    typename Cells>
void step_by_step(Cells& cells, float dt, int n_steps)
{
    Policy::before_steps(cells.n_max);
    Generic_forces<Pt> gen = Policy::gen(cells.n_replicas, cells.n_max);
    for (int s = 0; s < n_steps; s++) cells.template take_step<pw_int, pw_friction>(dt, gen);
}

// THE MODEL TABLE.  Factory is a pointer to a function that takes create's sizes and values and returns the .hip's
// interface; make_sim<Sim> is one (its arguments are deduced from the Factory it is stored as).
template<typename Factory>
struct Model {
    const char* name;
    Factory make;
};
template<typename S, typename... Args>
typename S::Interface* make_sim(Args... args)
{
    return new S{args...};
}
// (one row of a .hip's table; Sim is that file's)
#define YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, Policy) \
    { name, &ens_harness::make_sim<Sim<Pt, pw_int, pw_friction, Policy>> }
template<typename Factory>
const Model<Factory>* find(const Model<Factory>* table, int count, const char* name)
{
    for (int i = 0; i < count; i++)
        if (std::string(name) == table[i].name) return &table[i];
    return nullptr;
}
template<typename Factory>
const char* name_at(const Model<Factory>* table, int count, int i)
{
    return (i >= 0 && i < count) ? table[i].name : nullptr;
}
// The end of every create, after its own checks: -1 for a name the table does not hold, else a new handle.
template<typename Factory, typename Handle, typename... Args>
int create(const Model<Factory>* table, int count, const char* name, Handle** out, Args... args)
{
    const Model<Factory>* model = find(table, count, name);
    if (!model) return -1;
    Handle* e = new Handle;
    e->p.reset(model->make(args...));
    *out = e;
    return 0;
}

// THE ENTRY POINTS' BODIES.  Argument checks first, then ya_device_synchronize, then the copy.
inline int set_h_n(Replicas& s, int r, int n)
{
    if (r < 0 || r >= s.n_replicas() || n < 0 || n > s.n_max()) return -3;
    s.h_n()[r] = n;
    return 0;
}
inline int get_h_n(Replicas& s, int r)
{
    if (r < 0 || r >= s.n_replicas()) return -3;
    return s.h_n()[r];
}
inline int get_d_n(Replicas& s, int r)
{
    if (r < 0 || r >= s.n_replicas()) return -3;
    return s.get_d_n(r);
}
inline int copy_to_device(Replicas& s)
{
    s.copy_to_device();
    return 0;
}
inline int copy_to_host(Replicas& s)
{
    s.copy_to_host();
    return 0;
}
// (the Gabriel form's; the all-pairs and the grid take_steps return a count)
template<typename Interface>
int take_steps(Interface& s, float dt, int n_steps)
{
    s.take_steps(dt, n_steps);
    return 0;
}
inline int synchronize()
{
    YA_CHECK(ya_device_synchronize());
    return 0;
}
inline int set_fixed(Replicas& s, int mode, int local_point)
{
    if (mode < 0 || mode > 2) return -3;
    if (mode != 0 && (local_point < 0 || local_point >= s.n_max())) return -3;
    s.set_fixed(mode, local_point);
    return 0;
}
inline int get_old_v(Replicas& s, float* out)
{
    if (!out) return -3;
    YA_CHECK(ya_device_synchronize());
    YA_CHECK(ya_memcpy_d2h(out, s.d_old_v(), (size_t)s.n_replicas() * s.n_max() * 3 * sizeof(float)));
    return 0;
}
inline int set_old_v(Replicas& s, const float* in)
{
    if (!in) return -3;
    YA_CHECK(ya_device_synchronize());
    YA_CHECK(ya_memcpy_h2d(s.d_old_v(), in, (size_t)s.n_replicas() * s.n_max() * 3 * sizeof(float)));
    return 0;
}
// The two all-pairs forms' set_param: -2 for a name that is none of the four.
inline int set_tile_param(Tile_replicas& s, const char* name, double v)
{
    if (!name) return -3;
    if (std::string(name) == "tile_lanes") {
        const int lanes = (int)v;
        if (lanes != 0 && lanes != 1 && lanes != 16 && lanes != 64) return -3;
        s.set_lanes(lanes);
        return 0;
    }
    if (std::string(name) == "whole_steps") {
        if (v != -1 && v != 0 && v != 1) return -3;
        s.set_whole_steps((int)v);
        return 0;
    }
    if (std::string(name) == "steps_per_launch") {
        if (!(v >= 1 && v <= 0x7fffffff) || v != (double)(int)v) return -3;
        s.set_steps_per_launch((int)v);
        return 0;
    }
    if (std::string(name) == "whole_step_lanes") {
        if (v != 0 && v != 1 && v != 4 && v != 16 && v != 64) return -3;
        s.set_whole_step_lanes((int)v);
        return 0;
    }
    return -2;
}
// "lds_step_lanes" and "lds_step_lanes_used" of the two grid forms that step from LDS (Ensemble<Pt, Grid_solver>::
// lds_step_lanes, lds_step_lanes_used): Interface declares set_lds_step_lanes and lds_step_lanes_used.  The second
// name is THE GETTER: set_param with it sets nothing and returns the lanes of the last launch from LDS (0, 1, 4, 16 or
// 64; the value handed over must be 0).  It travels through set_param because the libraries' exported functions are
// held to an exact list.
inline bool lds_lanes_name(const std::string& name) { return name == "lds_step_lanes" || name == "lds_step_lanes_used"; }
template<typename Interface>
int lds_lanes_param(Interface& s, const std::string& name, double v)
{
    if (name == "lds_step_lanes_used") return v == 0 ? s.lds_step_lanes_used() : -3;
    if (v != 0 && v != 1 && v != 4 && v != 16 && v != 64) return -3;
    s.set_lds_step_lanes((int)v);
    return 0;
}
inline int set_cube_size(Grid_replicas& s, float cube_size)
{
    if (!(cube_size > 0)) return -3;
    s.set_cube_size(cube_size);
    return 0;
}
inline int status(Grid_replicas& s, int r, int clear)
{
    if (r < 0 || r >= s.n_replicas()) return -3;
    YA_CHECK(ya_device_synchronize());
    return s.status(r, clear != 0);
}
// Grid's cube_start / cube_end from a replica's n_cubes + 1 offs: an empty cube is -1 / -2, and every cube of a grid
// that was never built (offs[n_cubes] < 0) -1 / -1, which is what a fresh Grid holds.  Host arithmetic only.
inline void offs_to_start_end(const int* offs, size_t n_cubes, int* cube_start, int* cube_end)
{
    const bool built = offs[n_cubes] >= 0;
    for (size_t c = 0; c < n_cubes; c++) {
        const bool some = built && offs[c + 1] > offs[c];
        if (cube_start) cube_start[c] = some ? offs[c] : -1;
        if (cube_end) cube_end[c] = some ? offs[c + 1] - 1 : (built ? -2 : -1);
    }
}
inline int get_grid(Grid_replicas& s, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    if (r < 0 || r >= s.n_replicas()) return -3;
    const size_t n_max = s.n_max(), n_cubes = s.n_cubes();
    YA_CHECK(ya_device_synchronize());
    if (cube_id) YA_CHECK(ya_memcpy_d2h(cube_id, s.d_cube_id() + r * n_max, n_max * sizeof(int)));
    if (point_id) YA_CHECK(ya_memcpy_d2h(point_id, s.d_point_id() + r * n_max, n_max * sizeof(int)));
    if (cube_start || cube_end) {  // (not on the step's path)
        std::vector<int> offs(n_cubes + 1);
        YA_CHECK(ya_memcpy_d2h(offs.data(), s.d_offs() + r * (n_cubes + 1), offs.size() * sizeof(int)));
        offs_to_start_end(offs.data(), n_cubes, cube_start, cube_end);
    }
    return 0;
}

}  // namespace ens_harness

// (the wrapper of the declared name is declared as that name is; the `_plain` twin's is not)
YA_STATELESS_FRICTION(float3, ens_harness::friction_by_local_id<models::ids_friction>)
