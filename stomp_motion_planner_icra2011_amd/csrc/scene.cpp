// scene.cpp -- stomp_scene: a distance field kept in two layers over the caller's device buffer.
// The field is a capped squared distance, and for two sets of marks A and B
//     min(d2(A u B), cap^2) = min(min(d2(A), cap^2), min(d2(B), cap^2))
// holds exactly in integers, while a cell further than cap cells from every mark of B keeps A's
// value.  So the static layer (A: shelves, walls) is built once and kept, and a request's dynamic
// set (B: the robot's own bodies, the sensor points) costs an exact transform over the bounding
// window of B's marks grown by cap, a min merge over that window and a restore of the cells the
// previous window covered and the new one does not -- bit for bit stomp_sdf_build_objects of the
// static inputs followed by the dynamic ones.  Host side here: the window bound (scene_bound),
// the staging and the workspace; the kernels are k_sdf.hip's.
#include "engine_internal.h"

#include <algorithm>

#include "sdf_lattice.h"

using namespace stomp;

struct stomp_scene {
    int device = 0;
    int n[3] = {0, 0, 0};
    double o[3] = {0, 0, 0};
    double res = 0;
    int cap = 0;
    unsigned short* field = nullptr;   // the caller's buffer
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool ready = false;                // the device side exists (made by the first accepted set_static)
    bool has_static = false;
    unsigned short* stat = nullptr;    // the static layer, [n]
    unsigned char* ws = nullptr;       // window workspace: a, b (u16 each) and the marks, 5 B per cell
    size_t ws_cells = 0;
    double* h_stage = nullptr;         // pinned: axis lists | hull planes | points
    double* d_stage = nullptr;
    size_t h_cap = 0, d_cap = 0;       // doubles
    hipEvent_t staged = nullptr;       // behind the last upload out of h_stage
    bool staged_pending = false;
    unsigned long long* d_cnt = nullptr;   // [0] points landed in this call, [1] stray marks (cumulative)
    unsigned long long* h_cnt = nullptr;   // pinned read-back of d_cnt
    SdfBox prev{};                     // the dynamic set's window in the field (n = 0: none)
    SdfBox last{};                     // the last call's window (info)
    long long restored = 0;
    long long allocs = 0;              // allocations made inside set_dynamic
};

namespace {

constexpr int kMargin = 1;   // cells added around every object's bound

long long cells_of(const SdfBox& b) { return (long long)b.n[0] * b.n[1] * b.n[2]; }

long long overlap(const SdfBox& a, const SdfBox& b)
{
    long long v = 1;
    for (int k = 0; k < 3; ++k) {
        const int lo = std::max(a.lo[k], b.lo[k]), hi = std::min(a.lo[k] + a.n[k], b.lo[k] + b.n[k]);
        v *= hi > lo ? hi - lo : 0;
    }
    return v;
}

// one axis of an object's bound: the cells [round(ulo) - margin, round(uhi) + margin] of the
// coordinates ulo <= uhi (in cells, as mark_cell rounds them) clipped to the grid; lo > hi when
// none is left.  A coordinate that is not a number gives the whole axis.
void axis_cells(int n, double ulo, double uhi, int& lo, int& hi)
{
    const double a = std::round(ulo) - kMargin, b = std::round(uhi) + kMargin;
    lo = !(a > 0.0) ? 0 : (a > (double)n ? n : (int)a);
    hi = !(b < (double)(n - 1)) ? n - 1 : (b < -1.0 ? -1 : (int)b);
}

// The bound of every cell the marking kernels can mark for these inputs, clipped to the grid:
// false when nothing can land.
//   environment boxes / cylinders: the lattice is an affine image of the per-axis coordinate
//     lists, so every point's cell coordinate lies between those of the eight corners (first /
//     last list entry per axis) taken through the object's frame by k_mark_lattice's expressions;
//   robot bodies and meshes: the world-aligned lattice (lo + i) res + pos, monotone in i, so the
//     first and last index per axis bound it;
//   points: the cells of the points that pass mark_cell's own in-grid test.
bool scene_bound(const int* n, const double* o, double res, const LatticeSetup& L, const double* points,
                 long long n_points, SdfBox& m)
{
    const double inv_res = 1.0 / res;
    int mlo[3] = {n[0], n[1], n[2]}, mhi[3] = {-1, -1, -1};
    bool any = false;
    auto take = [&](const double* ulo, const double* uhi) {
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            axis_cells(n[a], ulo[a], uhi[a], lo[a], hi[a]);
            if (lo[a] > hi[a]) return;
        }
        for (int a = 0; a < 3; ++a) {
            mlo[a] = std::min(mlo[a], lo[a]);
            mhi[a] = std::max(mhi[a], hi[a]);
        }
        any = true;
    };
    for (const SdfLatticeJob& j : L.jobs) {
        if (j.n[0] <= 0 || j.n[1] <= 0 || j.n[2] <= 0) continue;
        double ulo[3], uhi[3];
        if (j.type == kShapeBox || j.type == kShapeCylinder) {
            bool finite = true;
            for (int a = 0; a < 3; ++a) {
                ulo[a] = 1e300;
                uhi[a] = -1e300;
            }
            for (int c = 0; c < 8; ++c) {
                double p[3];
                for (int a = 0; a < 3; ++a)
                    p[a] = j.pos[a] - L.axes[(size_t)j.off[a] + (((c >> a) & 1) ? j.n[a] - 1 : 0)];
                for (int a = 0; a < 3; ++a) {
                    const double p2 = j.R[3 * a + 0] * p[0] + j.R[3 * a + 1] * p[1] + j.R[3 * a + 2] * p[2] + j.pos[a];
                    const double u = (p2 - o[a]) * inv_res;
                    finite = finite && std::isfinite(u);
                    ulo[a] = std::min(ulo[a], u);
                    uhi[a] = std::max(uhi[a], u);
                }
            }
            if (!finite)
                for (int a = 0; a < 3; ++a) ulo[a] = uhi[a] = std::nan("");
        } else {
            for (int a = 0; a < 3; ++a) {
                ulo[a] = (((j.lo[a] + 0) * j.res + j.pos[a]) - o[a]) * inv_res;
                uhi[a] = (((j.lo[a] + (j.n[a] - 1)) * j.res + j.pos[a]) - o[a]) * inv_res;
            }
        }
        take(ulo, uhi);
    }
    double plo[3] = {1e300, 1e300, 1e300}, phi[3] = {-1e300, -1e300, -1e300};
    bool landed = false;
    for (long long i = 0; i < n_points; ++i) {
        double r[3];
        bool in = true;
        for (int a = 0; a < 3; ++a) {
            r[a] = std::round((points[3 * i + a] - o[a]) * inv_res);
            in = in && r[a] >= 0.0 && r[a] < (double)n[a];
        }
        if (!in) continue;
        landed = true;
        for (int a = 0; a < 3; ++a) {
            plo[a] = std::min(plo[a], r[a]);
            phi[a] = std::max(phi[a], r[a]);
        }
    }
    if (landed) take(plo, phi);
    for (int a = 0; a < 3; ++a) {
        m.lo[a] = any ? mlo[a] : 0;
        m.n[a] = any ? mhi[a] - mlo[a] + 1 : 0;
    }
    return any;
}

// the bound grown by cap and clipped to the grid
SdfBox grown(const int* n, const SdfBox& m, int cap)
{
    SdfBox w{};
    if (cells_of(m) == 0) return w;
    for (int a = 0; a < 3; ++a) {
        const int lo = std::max(m.lo[a] - cap, 0), hi = std::min(m.lo[a] + m.n[a] - 1 + cap, n[a] - 1);
        w.lo[a] = lo;
        w.n[a] = hi - lo + 1;
    }
    return w;
}

int check_grid(int32_t nx, int32_t ny, int32_t nz, const double* origin, double res, double max_expansion, int* cap)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || !origin || !(res > 0))
        return fail(nullptr, STOMP_E_INVALID, "scene: invalid grid (sizes and resolution must be positive, origin not null)");
    const double capd = std::ceil(max_expansion / res);
    if (!(capd >= 0) || capd > 255)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "scene: max_expansion / resolution above 255 cells");
    *cap = (int)capd;
    return 0;
}

int check_lists(const stomp_shape* shapes, int32_t n_shapes, const double* points, int64_t n_points)
{
    if (n_shapes < 0 || n_points < 0) return fail(nullptr, STOMP_E_INVALID, "scene: negative object or point count");
    if ((n_shapes > 0 && !shapes) || (n_points > 0 && !points))
        return fail(nullptr, STOMP_E_INVALID, "scene: a count without its array");
    return 0;
}

void count_alloc(stomp_scene* s, bool dynamic)
{
    if (dynamic) ++s->allocs;
}

// the device side of a scene: made by the first accepted set_static, so that creating a scene and
// every refused call touch no device
int make_ready(stomp_scene* s)
{
    if (s->ready) return 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || s->device >= count)
        return fail(nullptr, STOMP_E_DEVICE, "scene: device %d is not one of the %d present", s->device, count);
    const size_t cells = (size_t)s->n[0] * s->n[1] * s->n[2];
    if (!s->stream) {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
            return fail(nullptr, STOMP_E_DEVICE, "scene: hipStreamCreate failed");
        s->own_stream = true;
    }
    if (!s->staged && hipEventCreateWithFlags(&s->staged, hipEventDisableTiming) != hipSuccess)
        return fail(nullptr, STOMP_E_DEVICE, "scene: hipEventCreate failed");
    if (!s->stat && hipMalloc((void**)&s->stat, cells * sizeof(unsigned short)) != hipSuccess)
        return fail(nullptr, STOMP_E_DEVICE, "scene: hipMalloc of the static layer failed");
    if (!s->d_cnt) {
        if (hipMalloc((void**)&s->d_cnt, 2 * sizeof(unsigned long long)) != hipSuccess)
            return fail(nullptr, STOMP_E_DEVICE, "scene: hipMalloc failed");
        if (hipMemsetAsync(s->d_cnt, 0, 2 * sizeof(unsigned long long), s->stream) != hipSuccess)
            return fail(nullptr, STOMP_E_DEVICE, "scene: hipMemset failed");
    }
    if (!s->h_cnt) {
        if (hipHostMalloc((void**)&s->h_cnt, 2 * sizeof(unsigned long long)) != hipSuccess)
            return fail(nullptr, STOMP_E_DEVICE, "scene: hipHostMalloc failed");
        s->h_cnt[0] = s->h_cnt[1] = 0;
    }
    s->ready = true;
    return 0;
}

// staging of `doubles` and a workspace of `wcells`, the pinned staging free again (the last upload
// has left it).  Growth is geometric; a device buffer is freed once the stream's work has read it.
int reserve(stomp_scene* s, size_t doubles, size_t wcells, bool dynamic)
{
    if (s->staged_pending && hipEventSynchronize(s->staged) != hipSuccess)
        return fail(nullptr, STOMP_E_DEVICE, "scene: staging wait failed");
    s->staged_pending = false;
    if (doubles > s->h_cap) {
        const size_t want = std::max(doubles, 2 * s->h_cap);
        if (s->h_stage) hipHostFree(s->h_stage);
        s->h_stage = nullptr;
        s->h_cap = hipHostMalloc((void**)&s->h_stage, want * sizeof(double)) == hipSuccess ? want : 0;
        if (!s->h_cap) return fail(nullptr, STOMP_E_DEVICE, "scene: hipHostMalloc failed");
        count_alloc(s, dynamic);
    }
    if (doubles > s->d_cap) {
        const size_t want = std::max(doubles, 2 * s->d_cap);
        if (s->d_stage) {
            hipStreamSynchronize(s->stream);
            hipFree(s->d_stage);
        }
        s->d_stage = nullptr;
        s->d_cap = hipMalloc((void**)&s->d_stage, want * sizeof(double)) == hipSuccess ? want : 0;
        if (!s->d_cap) return fail(nullptr, STOMP_E_DEVICE, "scene: hipMalloc failed");
        count_alloc(s, dynamic);
    }
    if (wcells > s->ws_cells) {
        const size_t cells = (size_t)s->n[0] * s->n[1] * s->n[2];
        const size_t want = std::min(std::max(wcells, 2 * s->ws_cells), cells);
        if (s->ws) {
            hipStreamSynchronize(s->stream);
            hipFree(s->ws);
        }
        s->ws = nullptr;
        s->ws_cells = hipMalloc((void**)&s->ws, want * 5) == hipSuccess ? want : 0;
        if (!s->ws_cells) return fail(nullptr, STOMP_E_DEVICE, "scene: hipMalloc of the window workspace failed");
        count_alloc(s, dynamic);
    }
    return 0;
}

// One layer's inputs onto the stream.  Static: the window is the grid, the last pass writes the
// static layer and the field.  Dynamic: the window is the grown bound, the last pass merges.
int set_layer(stomp_scene* s, const stomp_shape* shapes, int32_t n_shapes, const double* points, int64_t n_points,
              int64_t* marked, bool dynamic)
{
    if (!s) return fail(nullptr, STOMP_E_INVALID, "scene: null scene");
    if (int rc = check_lists(shapes, n_shapes, points, n_points)) return rc;
    if (dynamic && !s->has_static) return fail(nullptr, STOMP_E_INVALID, "scene: set_dynamic before any set_static");
    LatticeSetup L;
    if (int rc = lattice_setup(shapes, n_shapes, s->res, L)) return rc;
    SdfBox m{}, w{};
    if (dynamic) {
        scene_bound(s->n, s->o, s->res, L, points, n_points, m);
        w = grown(s->n, m, s->cap);
    } else {
        for (int a = 0; a < 3; ++a) m.n[a] = w.n[a] = s->n[a];
    }
    // ---- everything below touches the device
    DeviceGuard dg(s->device);
    if (int rc = make_ready(s)) return rc;
    const size_t na = L.axes.size(), np = L.mesh_planes.size(), nq = (size_t)n_points * 3;
    if (int rc = reserve(s, na + np + nq, (size_t)cells_of(w), dynamic)) return rc;
    hipStream_t st = s->stream;
    hipError_t err = hipSuccess;
    const double* d_axes = s->d_stage;
    const double* d_planes = s->d_stage + na;
    const double* d_pts = s->d_stage + na + np;
    if (na + np + nq > 0) {
        if (na) std::memcpy(s->h_stage, L.axes.data(), na * sizeof(double));
        if (np) std::memcpy(s->h_stage + na, L.mesh_planes.data(), np * sizeof(double));
        if (nq) std::memcpy(s->h_stage + na + np, points, nq * sizeof(double));
        err = hipMemcpyAsync(s->d_stage, s->h_stage, (na + np + nq) * sizeof(double), hipMemcpyHostToDevice, st);
        if (err == hipSuccess) err = hipEventRecord(s->staged, st);
        if (err == hipSuccess) s->staged_pending = true;
    }
    resolve_mesh_planes(L.jobs, d_planes);
    unsigned short* a = (unsigned short*)s->ws;
    unsigned short* b = a + s->ws_cells;
    unsigned char* occ = s->ws + 4 * s->ws_cells;
    const long long wcells = cells_of(w);
    if (err == hipSuccess) err = hipMemsetAsync(s->d_cnt, 0, sizeof(unsigned long long), st);
    if (err == hipSuccess && wcells > 0) err = hipMemsetAsync(occ, 0, (size_t)wcells, st);
    if (err != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "scene: %s", hipGetErrorString(err));
    long long restored = 0;
    if (dynamic && cells_of(s->prev) > 0) {
        restored = cells_of(s->prev) - overlap(s->prev, w);
        if (restored > 0) launch_restore_box(s->n, s->prev, w, s->stat, s->field, st);
    }
    SdfMarkArgs g{};
    for (int k = 0; k < 3; ++k) {
        g.n[k] = s->n[k];
        g.o[k] = s->o[k];
        g.wlo[k] = w.lo[k];
        g.wn[k] = w.n[k];
    }
    g.inv_res = 1.0 / s->res;
    g.occ = occ;
    g.marked = s->d_cnt;
    g.stray = s->d_cnt + 1;
    launch_mark_points_window(d_pts, n_points, g, st);
    for (const SdfLatticeJob& j : L.jobs) launch_mark_lattice_window(j, d_axes, g, st);
    if (wcells > 0) {
        SdfWindowArgs A{};
        for (int k = 0; k < 3; ++k) A.gn[k] = s->n[k];
        A.w = w;
        A.m = m;
        A.cap = s->cap;
        A.occ = occ;
        A.a = a;
        A.b = b;
        A.stat = s->stat;
        A.field = s->field;
        launch_edt_box(A, dynamic, st);
    }
    err = hipGetLastError();
    if (err == hipSuccess && marked) {
        err = hipMemcpyAsync(s->h_cnt, s->d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
    }
    // the launches are on the stream: the scene's record follows them whatever the read-back says
    s->has_static = true;
    s->prev = dynamic ? w : SdfBox{};
    s->last = w;
    s->restored = restored;
    if (err != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "scene: %s", hipGetErrorString(err));
    if (marked) *marked = (int64_t)s->h_cnt[0];
    return 0;
}

}  // namespace

extern "C" {

int stomp_scene_create(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double* origin, double resolution,
                       double max_expansion, uint16_t* field_device, void* stream, stomp_scene** out)
{
    if (!out) return fail(nullptr, STOMP_E_INVALID, "scene: null out");
    *out = nullptr;
    int cap = 0;
    if (int rc = check_grid(nx, ny, nz, origin, resolution, max_expansion, &cap)) return rc;
    if (!field_device) return fail(nullptr, STOMP_E_INVALID, "scene: null field");
    if (device < 0) return fail(nullptr, STOMP_E_INVALID, "scene: negative device");
    stomp_scene* s = new stomp_scene();
    s->device = device;
    s->n[0] = nx;
    s->n[1] = ny;
    s->n[2] = nz;
    for (int a = 0; a < 3; ++a) s->o[a] = origin[a];
    s->res = resolution;
    s->cap = cap;
    s->field = field_device;
    s->stream = (hipStream_t)stream;
    *out = s;
    return 0;
}

int stomp_scene_set_static(stomp_scene* s, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                           int64_t n_points, int64_t* marked)
{
    return set_layer(s, shapes, n_shapes, points, n_points, marked, false);
}

int stomp_scene_set_dynamic(stomp_scene* s, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                            int64_t n_points, int64_t* marked)
{
    return set_layer(s, shapes, n_shapes, points, n_points, marked, true);
}

int stomp_scene_window(int32_t nx, int32_t ny, int32_t nz, const double* origin, double resolution,
                       double max_expansion, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                       int64_t n_points, int32_t lo[3], int32_t hi[3])
{
    int cap = 0;
    if (int rc = check_grid(nx, ny, nz, origin, resolution, max_expansion, &cap)) return rc;
    if (!lo || !hi) return fail(nullptr, STOMP_E_INVALID, "scene: null window");
    if (int rc = check_lists(shapes, n_shapes, points, n_points)) return rc;
    LatticeSetup L;
    if (int rc = lattice_setup(shapes, n_shapes, resolution, L)) return rc;
    const int n[3] = {nx, ny, nz};
    SdfBox m{};
    scene_bound(n, origin, resolution, L, points, n_points, m);
    const SdfBox w = grown(n, m, cap);
    for (int a = 0; a < 3; ++a) {
        lo[a] = w.lo[a];
        hi[a] = w.lo[a] + w.n[a] - 1;
    }
    return 0;
}

int stomp_scene_info(stomp_scene* s, int64_t info[10])
{
    if (!s || !info) return fail(nullptr, STOMP_E_INVALID, "scene: null argument");
    if (s->ready) {
        DeviceGuard dg(s->device);
        hipError_t err = hipMemcpyAsync(s->h_cnt + 1, s->d_cnt + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                        s->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
        if (err != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "scene: %s", hipGetErrorString(err));
    }
    for (int a = 0; a < 3; ++a) {
        info[a] = s->last.lo[a];
        info[3 + a] = s->last.lo[a] + s->last.n[a] - 1;
    }
    info[6] = cells_of(s->last);
    info[7] = s->restored;
    info[8] = s->ready ? (int64_t)s->h_cnt[1] : 0;
    info[9] = s->allocs;
    return 0;
}

void stomp_scene_destroy(stomp_scene* s)
{
    if (!s) return;
    if (s->ready || s->stream) {
        DeviceGuard dg(s->device);
        if (s->stream) hipStreamSynchronize(s->stream);
        if (s->staged) hipEventDestroy(s->staged);
        if (s->stat) hipFree(s->stat);
        if (s->ws) hipFree(s->ws);
        if (s->d_stage) hipFree(s->d_stage);
        if (s->d_cnt) hipFree(s->d_cnt);
        if (s->h_stage) hipHostFree(s->h_stage);
        if (s->h_cnt) hipHostFree(s->h_cnt);
        if (s->own_stream) hipStreamDestroy(s->stream);
    }
    delete s;
}

}  // extern "C"
