// sdf_build.cpp -- the distance-field builders of the C ABI (stomp_sdf_build,
// stomp_sdf_build_objects): the host prepares the per-object lattices and the meshes' hull planes,
// the marking and the distance transform run on the device (k_sdf.hip).  No engine is involved.
#include "stomp_engine.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>

#include "kernels.h"
#include "sdf_lattice.h"

namespace stomp {
int fail(stomp_engine* e, int code, const char* fmt, ...);   // engine.cpp; here always without an engine
}

using namespace stomp;

// bodies::ConvexMesh's convex hull (third party: qhull in geometric_shapes) as its supporting
// planes, appended to `planes` as (n, d) with unit outward n and n.x + d = 0 on the face; the steps
// of oracle/sdf_oracle.c so_hull_planes, restated in C++ (same expressions, so the same planes):
// merge vertices with identical coordinates (first index kept), incremental hull of the unique
// vertices in index order (first tetrahedron, then each vertex more than eps outside a face
// replaces the faces it sees by a fan over their horizon), faces with the same plane (n . n' >
// 1 - 1e-12, |d - d'| <= eps) merged into facets, each facet's plane spanned by the first
// non-collinear triple of its vertices (|u x w| > 1e-12 |u| |w|) that leaves every hull vertex
// within eps on one side, facets in the order of those triples.  eps = 1e-9 (1 + max |coordinate|).
// O(V log V + V F).  Returns the number of planes (-1: no volume).
namespace hull {
struct Face {
    int v[3];
    double n[3], d;
    int alive;
};
inline const double* at(const double* V, int i) { return V + 3 * (size_t)i; }
inline bool plane3(const double* V, int a, int b, int c, double* n, double* d)
{
    const double* A = at(V, a);
    const double* B = at(V, b);
    const double* C = at(V, c);
    const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double w[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double lu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double lw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(len > 1e-12 * lu * lw) || !(len > 0.0)) return false;
    n[0] /= len;
    n[1] /= len;
    n[2] /= len;
    *d = -(n[0] * A[0] + n[1] * A[1] + n[2] * A[2]);
    return true;
}
inline double sdist(const double* n, double d, const double* p) { return n[0] * p[0] + n[1] * p[1] + n[2] * p[2] + d; }
inline uint64_t edge_key(int a, int b) { return ((uint64_t)(unsigned)a << 32) | (unsigned)b; }

// the vertices with distinct coordinates (first index kept), in index order
static std::vector<int> unique_vertices(const double* V, int nv)
{
    std::vector<int> ord(nv), uq;
    for (int i = 0; i < nv; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](int i, int j) {
        for (int k = 0; k < 3; ++k) {
            const double x = V[3 * (size_t)i + k], y = V[3 * (size_t)j + k];
            if (x != y) return x < y;
        }
        return i < j;
    });
    for (int i = 0; i < nv; ++i) {
        const double* p = at(V, ord[i]);
        if (i > 0) {
            const double* q = at(V, ord[i - 1]);
            if (p[0] == q[0] && p[1] == q[1] && p[2] == q[2]) continue;
        }
        uq.push_back(ord[i]);
    }
    std::sort(uq.begin(), uq.end());
    return uq;
}

// the hull under construction: its faces (dead ones stay in place), the face of each directed
// edge, and which vertices it has taken
struct Hull {
    std::vector<Face> F;
    std::unordered_map<uint64_t, int> em;
    std::vector<unsigned char> onhull;
};

// the first tetrahedron: the first vertex, the one farthest from it, the one farthest from their
// line, the one farthest from their plane (each more than eps away); false: no volume
static bool first_tetrahedron(const double* V, const std::vector<int>& uq, double eps, Hull& H)
{
    const int nu = (int)uq.size();
    const int a = uq[0];
    int b = -1, c = -1, e = -1;
    double best = eps;
    for (int i = 1; i < nu; ++i) {
        const double* p = at(V, uq[i]);
        const double* A = at(V, a);
        const double dx = p[0] - A[0], dy = p[1] - A[1], dz = p[2] - A[2];
        const double r = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (r > best) { best = r; b = uq[i]; }
    }
    if (b < 0) return false;
    best = eps;
    for (int i = 1; i < nu; ++i) {
        const double* A = at(V, a);
        const double* B = at(V, b);
        const double* p = at(V, uq[i]);
        const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
        const double w[3] = {p[0] - A[0], p[1] - A[1], p[2] - A[2]};
        const double x[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double r = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) / std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (r > best) { best = r; c = uq[i]; }
    }
    if (c < 0) return false;
    double n[3], d;
    if (!plane3(V, a, b, c, n, &d)) return false;
    best = eps;
    for (int i = 1; i < nu; ++i) {
        const double r = std::fabs(sdist(n, d, at(V, uq[i])));
        if (r > best) { best = r; e = uq[i]; }
    }
    if (e < 0) return false;
    const int tet[4][3] = {{a, b, c}, {a, e, b}, {b, e, c}, {c, e, a}};
    double ctr[3];
    for (int k = 0; k < 3; ++k) ctr[k] = (at(V, a)[k] + at(V, b)[k] + at(V, c)[k] + at(V, e)[k]) / 4.0;
    for (int f = 0; f < 4; ++f) {
        Face h;
        h.v[0] = tet[f][0]; h.v[1] = tet[f][1]; h.v[2] = tet[f][2];
        if (!plane3(V, h.v[0], h.v[1], h.v[2], h.n, &h.d)) return false;
        if (sdist(h.n, h.d, ctr) > 0.0) {
            std::swap(h.v[1], h.v[2]);
            if (!plane3(V, h.v[0], h.v[1], h.v[2], h.n, &h.d)) return false;
        }
        h.alive = 1;
        H.F.push_back(h);
        for (int k = 0; k < 3; ++k) H.em[edge_key(h.v[k], h.v[(k + 1) % 3])] = f;
    }
    H.onhull[a] = H.onhull[b] = H.onhull[c] = H.onhull[e] = 1;
    return true;
}

// the remaining vertices in index order: one more than eps outside a face replaces the faces it
// sees by a fan over their horizon
static void add_vertices(const double* V, const std::vector<int>& uq, double eps, Hull& H)
{
    std::vector<Face>& F = H.F;
    std::unordered_map<uint64_t, int>& em = H.em;
    std::vector<unsigned char>& onhull = H.onhull;
    const int nu = (int)uq.size();
    std::vector<int> vis, hor;
    for (int i = 1; i < nu; ++i) {
        const int p = uq[i];
        if (onhull[p]) continue;
        const double* P = at(V, p);
        vis.clear();
        for (int f = 0; f < (int)F.size(); ++f)
            if (F[f].alive && sdist(F[f].n, F[f].d, P) > eps) vis.push_back(f);
        if (vis.empty()) continue;
        for (int f : vis) F[f].alive = 2;
        hor.clear();
        for (int f : vis)
            for (int k = 0; k < 3; ++k) {
                const int ea = F[f].v[k], eb = F[f].v[(k + 1) % 3];
                const auto it = em.find(edge_key(eb, ea));
                if (it != em.end() && F[it->second].alive == 2) continue;
                hor.push_back(ea);
                hor.push_back(eb);
            }
        for (int f : vis) F[f].alive = 0;
        for (size_t q = 0; q < hor.size(); q += 2) {
            Face h;
            h.v[0] = hor[q]; h.v[1] = hor[q + 1]; h.v[2] = p;
            h.alive = 1;
            if (!plane3(V, h.v[0], h.v[1], h.v[2], h.n, &h.d)) { h.n[0] = h.n[1] = h.n[2] = 0.0; h.d = 0.0; }
            const int id = (int)F.size();
            F.push_back(h);
            for (int k = 0; k < 3; ++k) em[edge_key(h.v[k], h.v[(k + 1) % 3])] = id;
        }
        onhull[p] = 1;
    }
}

struct Facet {
    int t[3];
    double n[3], d;
};

// faces with the same plane merged into facets, each facet's plane spanned by the first
// non-collinear triple of its vertices that leaves every hull vertex within eps on one side
static std::vector<Facet> facets(const double* V, const std::vector<int>& uq, double eps, Hull& H)
{
    const std::vector<Face>& F = H.F;
    std::vector<unsigned char>& onhull = H.onhull;
    const int nu = (int)uq.size();
    for (const Face& f : F)
        if (f.alive)
            for (int k = 0; k < 3; ++k) onhull[f.v[k]] = 2;
    std::vector<int> hullv;
    for (int i = 0; i < nu; ++i)
        if (onhull[uq[i]] == 2) hullv.push_back(uq[i]);
    std::vector<Facet> fc;
    std::vector<int> grp(F.size(), -1), fv;
    const int nf = (int)F.size();
    for (int f = 0; f < nf; ++f) {
        if (!F[f].alive || grp[f] >= 0) continue;
        fv.clear();
        for (int g = f; g < nf; ++g) {
            if (!F[g].alive || grp[g] >= 0) continue;
            if (g != f && !(F[f].n[0] * F[g].n[0] + F[f].n[1] * F[g].n[1] + F[f].n[2] * F[g].n[2] > 1.0 - 1e-12 &&
                            std::fabs(F[f].d - F[g].d) <= eps))
                continue;
            grp[g] = f;
            for (int k = 0; k < 3; ++k) fv.push_back(F[g].v[k]);
        }
        std::sort(fv.begin(), fv.end());
        fv.erase(std::unique(fv.begin(), fv.end()), fv.end());
        const int mu = (int)fv.size();
        bool found = false;
        for (int x = 0; x < mu && !found; ++x)
            for (int y = x + 1; y < mu && !found; ++y)
                for (int z = y + 1; z < mu && !found; ++z) {
                    double n[3], d;
                    if (!plane3(V, fv[x], fv[y], fv[z], n, &d)) continue;
                    double smax = -1e300, smin = 1e300;
                    for (int q : hullv) {
                        const double sd = sdist(n, d, at(V, q));
                        if (sd > smax) smax = sd;
                        if (sd < smin) smin = sd;
                    }
                    if (smax <= eps) {
                    } else if (smin >= -eps) {
                        n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; d = -d;
                    } else {
                        continue;
                    }
                    fc.push_back(Facet{{fv[x], fv[y], fv[z]}, {n[0], n[1], n[2]}, d});
                    found = true;
                }
    }
    return fc;
}

}  // namespace hull

static int hull_planes(const double* V, int nv, std::vector<double>& planes)
{
    using namespace hull;
    if (nv < 4) return -1;
    double ext = 0.0;
    for (int i = 0; i < 3 * nv; ++i)
        if (std::fabs(V[i]) > ext) ext = std::fabs(V[i]);
    const double eps = 1e-9 * (1.0 + ext);
    const std::vector<int> uq = unique_vertices(V, nv);
    if (uq.size() < 4) return -1;
    Hull H;
    H.onhull.assign(nv, 0);
    if (!first_tetrahedron(V, uq, eps, H)) return -1;
    add_vertices(V, uq, eps, H);
    std::vector<Facet> fc = facets(V, uq, eps, H);
    std::sort(fc.begin(), fc.end(), [](const Facet& a, const Facet& b) {
        for (int k = 0; k < 3; ++k)
            if (a.t[k] != b.t[k]) return a.t[k] < b.t[k];
        return false;
    });
    const size_t first = planes.size();
    int np = 0;
    for (const Facet& q : fc) {
        bool dup = false;
        for (int p2 = 0; p2 < np && !dup; ++p2) {
            const double* e = planes.data() + first + 4 * p2;
            dup = q.n[0] * e[0] + q.n[1] * e[1] + q.n[2] * e[2] > 1.0 - 1e-12 && std::fabs(q.d - e[3]) <= eps;
        }
        if (dup) continue;
        planes.insert(planes.end(), {q.n[0], q.n[1], q.n[2], q.d});
        ++np;
    }
    if (np < 4) {
        planes.resize(first);
        return -1;
    }
    return np;
}

// the vertices' bounding-box centre and the largest distance of a vertex from it (bodies::
// ConvexMesh's bounding sphere before the pose; third party, parity unpinned)
static void mesh_box_sphere(const double* V, int nv, double* centre, double* radius)
{
    double lo[3] = {V[0], V[1], V[2]}, hi[3] = {V[0], V[1], V[2]};
    for (int q = 1; q < nv; ++q)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], V[3 * q + a]);
            hi[a] = std::max(hi[a], V[3 * q + a]);
        }
    for (int a = 0; a < 3; ++a) centre[a] = (lo[a] + hi[a]) / 2.0;
    double r2 = 0.0;
    for (int q = 0; q < nv; ++q) {
        const double dx = V[3 * q] - centre[0], dy = V[3 * q + 1] - centre[1], dz = V[3 * q + 2] - centre[2];
        const double s = dx * dx + dy * dy + dz * dz;
        if (s > r2) r2 = s;
    }
    *radius = std::sqrt(r2);
}

namespace stomp {

// btMatrix3x3::setRotation (bodies::Body::setPose) of the quaternion (x, y, z, w)
void body_basis(const double* q, double* B)
{
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const double dq = qx * qx + qy * qy + qz * qz + qw * qw;
    const double sc = 2.0 / dq;
    const double xs = qx * sc, ys = qy * sc, zs = qz * sc;
    const double wx = qw * xs, wy = qw * ys, wz = qw * zs;
    const double xx = qx * xs, xy = qx * ys, xz = qx * zs;
    const double yy = qy * ys, yz = qy * zs, zz = qz * zs;
    const double M[9] = {1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx,
                         xz - wy, yz + wx, 1.0 - (xx + yy)};
    std::memcpy(B, M, sizeof M);
}

// bodies::*::computeBoundingSphere of a STOMP_BODY_* shape posed with basis B at its position
// (padding folded into dims; a mesh's: the sphere around its vertices' bounding-box centre, grown
// by the padding).  Returns false for any other type, or a mesh without its vertices.
bool body_bounding_sphere(const stomp_shape& sh, const double* B, double* centre, double* radius)
{
    const double* d = sh.dims;
    for (int a = 0; a < 3; ++a) centre[a] = sh.position[a];
    if (sh.type == STOMP_BODY_SPHERE) {
        *radius = d[0];
    } else if (sh.type == STOMP_BODY_BOX) {
        const double a = d[0] / 2.0, b = d[1] / 2.0, c = d[2] / 2.0;
        *radius = std::sqrt(a * a + b * b + c * c);
    } else if (sh.type == STOMP_BODY_CYLINDER) {
        const double h = d[1] / 2.0;
        *radius = std::sqrt(d[0] * d[0] + h * h);
    } else if (sh.type == STOMP_BODY_MESH) {
        if (!sh.vertices || sh.num_vertices < 1) return false;
        double bc[3], rb;
        mesh_box_sphere(sh.vertices, sh.num_vertices, bc, &rb);
        for (int a = 0; a < 3; ++a)
            centre[a] = B[3 * a] * bc[0] + B[3 * a + 1] * bc[1] + B[3 * a + 2] * bc[2] + sh.position[a];
        *radius = rb + d[0];
    } else {
        return false;
    }
    return true;
}

// StompCollisionSpace::setStartState's per-object lattices (stomp_collision_space.cpp:199-297,
// 564-650): the environment objects' coordinate lists by the reference's own running-sum loops,
// the robot bodies' and meshes' bounding-sphere lattices, the meshes' hull planes
int lattice_setup(const stomp_shape* shapes, int n_shapes, double res, LatticeSetup& out)
{
    std::vector<double>& axes = out.axes;
    std::vector<double>& mesh_planes = out.mesh_planes;   // every mesh's hull planes, 4 doubles each
    std::vector<SdfLatticeJob>& jobs = out.jobs;
    const long long kMaxLattice = 1LL << 31;
    for (int s = 0; s < n_shapes; ++s) {
        const stomp_shape& sh = shapes[s];
        SdfLatticeJob j{};
        j.type = sh.type;
        j.res = res;
        for (int a = 0; a < 3; ++a) {
            j.pos[a] = sh.position[a];
            j.dims[a] = sh.dims[a];
        }
        const double qx = sh.orientation[0], qy = sh.orientation[1], qz = sh.orientation[2], qw = sh.orientation[3];
        if (sh.type == STOMP_SHAPE_BOX || sh.type == STOMP_SHAPE_CYLINDER) {
            // KDL::Rotation::Quaternion(x, y, z, w) (:243-246)
            const double x2 = qx * qx, y2 = qy * qy, z2 = qz * qz, w2 = qw * qw;
            const double R[9] = {w2 + x2 - y2 - z2, 2 * qx * qy - 2 * qw * qz, 2 * qx * qz + 2 * qw * qy,
                                 2 * qx * qy + 2 * qw * qz, w2 - x2 + y2 - z2, 2 * qy * qz - 2 * qw * qx,
                                 2 * qx * qz - 2 * qw * qy, 2 * qy * qz + 2 * qw * qx, w2 - x2 - y2 + z2};
            std::memcpy(j.R, R, sizeof R);
            const bool cyl = sh.type == STOMP_SHAPE_CYLINDER;
            const double* p = sh.position;
            const double* d = sh.dims;
            const double low[3] = {cyl ? p[0] - d[0] : p[0] - d[0] / 2.0, cyl ? p[1] - d[0] : p[1] - d[1] / 2.0,
                                   cyl ? p[2] - d[1] / 2.0 : p[2] - d[2] / 2.0};
            const double ext[3] = {cyl ? d[0] * 2.0 : d[0], cyl ? d[0] * 2.0 : d[1], cyl ? d[1] : d[2]};
            long long npts = 1;
            for (int a = 0; a < 3; ++a) {
                j.off[a] = (int)axes.size();
                // for (double x = xlow; x <= xlow + dim + resolution_; x += resolution_) (:255-257, 283-285)
                for (double x = low[a]; x <= low[a] + ext[a] + res; x += res) {
                    axes.push_back(x);
                    if ((long long)axes.size() - j.off[a] > kMaxLattice)
                        return fail(nullptr, STOMP_E_INVALID, "object %d: lattice too large", s);
                }
                j.n[a] = (int)axes.size() - j.off[a];
                npts *= j.n[a];
            }
            if (npts > kMaxLattice) return fail(nullptr, STOMP_E_INVALID, "object %d: lattice too large", s);
        } else if (sh.type >= STOMP_BODY_SPHERE && sh.type <= STOMP_BODY_MESH) {
            double B[9];
            body_basis(sh.orientation, B);
            std::memcpy(j.R, B, sizeof B);
            if (sh.type == STOMP_BODY_MESH) {
                // bodies::ConvexMesh: the convex hull of the vertices as planes, the lattice around
                // the bounding sphere of the vertices' bounding-box centre
                if (!sh.vertices || sh.num_vertices < 4)
                    return fail(nullptr, STOMP_E_INVALID, "mesh %d: needs at least 4 vertices", s);
                const int first = (int)mesh_planes.size() / 4;
                const int np = hull_planes(sh.vertices, sh.num_vertices, mesh_planes);
                if (np < 0) return fail(nullptr, STOMP_E_INVALID, "mesh %d: the vertices span no volume", s);
                j.nplanes = np;
                j.off[0] = first;   // plane offset, resolved to a device pointer below
            }
            double r, centre[3];   // bodies::*::computeBoundingSphere
            body_bounding_sphere(sh, B, centre, &r);
            if (sh.type == STOMP_BODY_MESH)
                for (int a = 0; a < 3; ++a) {
                    j.org[a] = sh.position[a];
                    j.pos[a] = centre[a];
                }
            long long npts = 1;
            for (int a = 0; a < 3; ++a) {
                const double c = centre[a];
                const double lo = ((c - r) - c) * (1.0 / res), hi = ((c + r) - c) * (1.0 / res);
                if (!(std::fabs(lo) < 1e9 && std::fabs(hi) < 1e9))
                    return fail(nullptr, STOMP_E_INVALID, "body %d: lattice too large", s);
                j.lo[a] = (int)lo;   // worldToGrid truncates (stomp_collision_space.h:230-234)
                j.n[a] = (int)hi - j.lo[a] + 1;
                if (j.n[a] < 0) j.n[a] = 0;
                npts *= j.n[a];
            }
            if (npts > kMaxLattice) return fail(nullptr, STOMP_E_INVALID, "body %d: lattice too large", s);
        } else {
            return fail(nullptr, STOMP_E_INVALID, "object %d: unknown type %d", s, sh.type);
        }
        jobs.push_back(j);
    }
    return 0;
}

void resolve_mesh_planes(std::vector<SdfLatticeJob>& jobs, const double* d_planes)
{
    for (SdfLatticeJob& j : jobs)
        if (j.type == kBodyMesh) {
            j.planes = d_planes + 4 * (size_t)j.off[0];
            j.off[0] = 0;
        }
}

}  // namespace stomp

extern "C" {

int stomp_attached_collision_points(const stomp_sphere* base, int32_t n_base, const stomp_attached_body* bodies,
                                    int32_t n_bodies, double clearance, stomp_sphere* out, int32_t capacity,
                                    int32_t* n_out)
{
    if (!out || !n_out || n_base < 0 || n_bodies < 0 || capacity < 0 || (n_base > 0 && !base) || (n_bodies > 0 && !bodies))
        return fail(nullptr, STOMP_E_INVALID, "attached collision points: null array or negative count");
    if (!(clearance > 0.0) || !std::isfinite(clearance))
        return fail(nullptr, STOMP_E_INVALID, "attached collision points: clearance not finite and positive");
    std::vector<stomp_sphere> added(n_bodies);
    for (int i = 0; i < n_bodies; ++i) {
        const stomp_shape& sh = bodies[i].shape;
        if (sh.type == STOMP_BODY_MESH && (!sh.vertices || sh.num_vertices < 4))
            return fail(nullptr, STOMP_E_INVALID, "mesh %d: needs at least 4 vertices", i);
        double B[9];
        body_basis(sh.orientation, B);
        stomp_sphere& sp = added[i];
        sp.segment = bodies[i].segment;
        sp.clearance = clearance;
        if (!body_bounding_sphere(sh, B, sp.pos, &sp.radius))
            return fail(nullptr, STOMP_E_INVALID, "attached body %d: type %d is no robot body shape", i, sh.type);
    }
    const int n = n_base + n_bodies;
    *n_out = n;
    if (capacity < n)
        return fail(nullptr, STOMP_E_INVALID, "attached collision points: %d entries needed, capacity %d", n, capacity);
    // each new sphere after the last sphere of its segment (the bodies of one segment in input
    // order); a segment the list has no sphere of: before the first sphere of a later segment
    std::vector<stomp_sphere> list(base, base + n_base);
    for (const stomp_sphere& sp : added) {
        size_t at = list.size();
        bool found = false;
        for (size_t k = list.size(); k-- > 0;)
            if (list[k].segment == sp.segment) { at = k + 1; found = true; break; }
        if (!found)
            for (size_t k = 0; k < list.size(); ++k)
                if (list[k].segment > sp.segment) { at = k; break; }
        list.insert(list.begin() + at, sp);
    }
    if (n) std::memcpy(out, list.data(), sizeof(stomp_sphere) * n);
    return 0;
}

int stomp_sdf_build(int32_t nx, int32_t ny, int32_t nz, const double* origin, double res, double max_expansion,
                    const double* boxes, int32_t n_boxes, const double* cyl, int32_t n_cyl, uint16_t* out, void* stream)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || !(res > 0) || !out) return fail(nullptr, STOMP_E_INVALID, "invalid grid");
    const int n[3] = {nx, ny, nz};
    const double capd = std::ceil(max_expansion / res);
    if (!(capd >= 0) || capd > 255) return fail(nullptr, STOMP_E_UNSUPPORTED, "max_expansion / resolution above 255 cells");
    const int cap = (int)capd;
    const int cap2 = cap * cap;
    auto range = [&](double lo, double hi, int a, int& i0, int& i1) {
        i0 = std::max((int)std::ceil((lo - origin[a]) / res), 0);
        i1 = std::min((int)std::floor((hi - origin[a]) / res), n[a] - 1);
    };
    std::vector<int> br;
    for (int b = 0; b < n_boxes; ++b) {
        const double* q = boxes + 6 * b;
        int r[6];
        bool empty = false;
        for (int a = 0; a < 3; ++a) {
            range(q[a] - q[3 + a] / 2.0, q[a] + q[3 + a] / 2.0, a, r[2 * a], r[2 * a + 1]);
            if (r[2 * a] > r[2 * a + 1]) empty = true;
        }
        if (!empty) br.insert(br.end(), r, r + 6);
    }
    const long long big = 1LL << 40;
    std::vector<long long> cd2;
    std::vector<int> cz;
    for (int c = 0; c < n_cyl; ++c) {
        const double* q = cyl + 5 * c;
        int z0, z1;
        range(q[2] - q[4] / 2.0, q[2] + q[4] / 2.0, 2, z0, z1);
        if (z0 > z1) continue;
        std::vector<std::pair<int, int>> disc;
        for (int i = 0; i < nx; ++i) {
            const double xs = origin[0] + i * res - q[0];
            for (int j = 0; j < ny; ++j) {
                const double ys = origin[1] + j * res - q[1];
                if (xs * xs + ys * ys <= q[3] * q[3]) disc.push_back({i, j});
            }
        }
        if (disc.empty()) continue;
        std::vector<long long> t((size_t)nx * ny, big);
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                long long best = big;
                for (auto& pq : disc) {
                    long long dx = i - pq.first, dy = j - pq.second;
                    long long v = dx * dx + dy * dy;
                    if (v < best) best = v;
                }
                t[(size_t)i * ny + j] = std::min(best, (long long)cap2);
            }
        cd2.insert(cd2.end(), t.begin(), t.end());
        cz.push_back(z0);
        cz.push_back(z1);
    }
    hipStream_t s = (hipStream_t)stream;
    int* d_b = nullptr;
    long long* d_c = nullptr;
    int* d_z = nullptr;
    if (!br.empty() && hipMalloc(&d_b, br.size() * sizeof(int)) != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "hipMalloc");
    if (!cd2.empty() && hipMalloc(&d_c, cd2.size() * sizeof(long long)) != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "hipMalloc");
    if (!cz.empty() && hipMalloc(&d_z, cz.size() * sizeof(int)) != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "hipMalloc");
    hipError_t cp = hipSuccess;
    if (d_b) cp = hipMemcpyAsync(d_b, br.data(), br.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (d_c && cp == hipSuccess) cp = hipMemcpyAsync(d_c, cd2.data(), cd2.size() * sizeof(long long), hipMemcpyHostToDevice, s);
    if (d_z && cp == hipSuccess) cp = hipMemcpyAsync(d_z, cz.data(), cz.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (cp != hipSuccess) {
        if (d_b) hipFree(d_b);
        if (d_c) hipFree(d_c);
        if (d_z) hipFree(d_z);
        return fail(nullptr, STOMP_E_DEVICE, "sdf build: %s", hipGetErrorString(cp));
    }
    launch_sdf_build(nx, ny, nz, cap2, d_b, (int)br.size() / 6, d_c, d_z, (int)cz.size() / 2, out, s);
    hipError_t st = hipStreamSynchronize(s);
    if (d_b) hipFree(d_b);
    if (d_c) hipFree(d_c);
    if (d_z) hipFree(d_z);
    if (st != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "sdf build: %s", hipGetErrorString(st));
    return 0;
}

// StompCollisionSpace::setStartState's fill (stomp_collision_space.cpp:154-297, 564-650): the
// per-object lattice is set up on the host (lattice_setup), the marking and the EDT run on the
// device (k_sdf.hip)
int stomp_sdf_build_objects(int32_t nx, int32_t ny, int32_t nz, const double* origin, double res,
                            double max_expansion, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                            int64_t n_points, uint16_t* out, int64_t* marked, void* stream)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || !(res > 0) || !out || !origin || n_shapes < 0 || n_points < 0 ||
        (n_shapes > 0 && !shapes) || (n_points > 0 && !points))
        return fail(nullptr, STOMP_E_INVALID, "invalid grid or object list");
    const double capd = std::ceil(max_expansion / res);
    if (!(capd >= 0) || capd > 255) return fail(nullptr, STOMP_E_UNSUPPORTED, "max_expansion / resolution above 255 cells");
    const int cap = (int)capd;
    LatticeSetup L;
    if (int rc = lattice_setup(shapes, n_shapes, res, L)) return rc;
    std::vector<double>& axes = L.axes;
    std::vector<double>& mesh_planes = L.mesh_planes;
    std::vector<SdfLatticeJob>& jobs = L.jobs;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)nx * ny * nz;
    unsigned char* occ = nullptr;
    unsigned short *a = nullptr, *b = nullptr;
    double *d_axes = nullptr, *d_pts = nullptr, *d_planes = nullptr;
    unsigned long long* d_marked = nullptr;
    auto cleanup = [&]() {
        if (occ) hipFree(occ);
        if (a) hipFree(a);
        if (b) hipFree(b);
        if (d_axes) hipFree(d_axes);
        if (d_pts) hipFree(d_pts);
        if (d_planes) hipFree(d_planes);
        if (d_marked) hipFree(d_marked);
    };
    if (hipMalloc(&occ, cells) != hipSuccess || hipMalloc(&a, cells * 2) != hipSuccess ||
        hipMalloc(&b, cells * 2) != hipSuccess || hipMalloc(&d_marked, sizeof(unsigned long long)) != hipSuccess ||
        (!axes.empty() && hipMalloc(&d_axes, axes.size() * sizeof(double)) != hipSuccess) ||
        (!mesh_planes.empty() && hipMalloc(&d_planes, mesh_planes.size() * sizeof(double)) != hipSuccess) ||
        (n_points > 0 && hipMalloc(&d_pts, (size_t)n_points * 3 * sizeof(double)) != hipSuccess)) {
        cleanup();
        return fail(nullptr, STOMP_E_DEVICE, "sdf build: hipMalloc");
    }
    resolve_mesh_planes(jobs, d_planes);
    hipError_t err = hipMemsetAsync(occ, 0, cells, st);
    if (err == hipSuccess) err = hipMemsetAsync(d_marked, 0, sizeof(unsigned long long), st);
    if (err == hipSuccess && d_axes)
        err = hipMemcpyAsync(d_axes, axes.data(), axes.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (err == hipSuccess && d_planes)
        err = hipMemcpyAsync(d_planes, mesh_planes.data(), mesh_planes.size() * sizeof(double), hipMemcpyHostToDevice,
                             st);
    if (err == hipSuccess && d_pts)
        err = hipMemcpyAsync(d_pts, points, (size_t)n_points * 3 * sizeof(double), hipMemcpyHostToDevice, st);
    if (err != hipSuccess) {
        cleanup();
        return fail(nullptr, STOMP_E_DEVICE, "sdf build: %s", hipGetErrorString(err));
    }
    SdfMarkArgs g{};
    g.n[0] = nx;
    g.n[1] = ny;
    g.n[2] = nz;
    for (int k = 0; k < 3; ++k) g.o[k] = origin[k];
    g.inv_res = 1.0 / res;
    g.occ = occ;
    g.marked = d_marked;
    launch_mark_points(d_pts, n_points, g, st);
    for (const SdfLatticeJob& j : jobs) launch_mark_lattice(j, d_axes, g, st);
    launch_edt(nx, ny, nz, cap, occ, a, b, out, st);
    unsigned long long nm = 0;
    err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(&nm, d_marked, sizeof nm, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    cleanup();
    if (err != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "sdf build: %s", hipGetErrorString(err));
    if (marked) *marked = (int64_t)nm;
    return 0;
}

}  // extern "C"
