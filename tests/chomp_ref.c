/*
 * tests/chomp_ref.c -- TEST INFRASTRUCTURE: a C99 restatement of the reference's covariant gradient
 * descent (CHOMP mode, use_chomp) on one trajectory, the CPU side of the stomp_chomp_* parity tests.
 * Reference paths are relative to stomp_motion_planner/.  It is compiled together with the
 * unchanged oracle (the #include below) to reach its FK frames, dm_sincos, field lookup, joint
 * limit passes and set-up products without copying them; nothing of the oracle is changed.
 *
 *   cr_build_quad_full     StompCost ctor + scale                stomp_cost.cpp:47-74, 99-105,
 *                                                                stomp_optimizer.cpp:100-125
 *   cr_field_gradient      distance_field getDistanceGradient    (third party; definition in DESIGN.md)
 *   cr_fk_all / cr_fk_one  performForwardKinematics              stomp_optimizer.cpp:618-709
 *                          JntToCartFull / Partial               treefksolverjointposaxis*.cpp
 *   potential gradient     getCollisionPointPotentialGradient    stomp_collision_space.h:193-228
 *   cr_jacobian_at         StompCollisionPoint::getJacobian      stomp_collision_point.h:120-136
 *   cr_smoothness          calculateSmoothnessIncrements         stomp_optimizer.cpp:403-411, stomp_cost.h:80-83
 *   cr_collision           calculateCollisionIncrements          stomp_optimizer.cpp:413-470
 *   cr_total               calculateTotalIncrements              stomp_optimizer.cpp:472-486
 *   cr_add                 addIncrementsToTrajectory             stomp_optimizer.cpp:488-506
 *   cr_step_one            doChompOptimization                   stomp_optimizer.cpp:208-247
 *   cr_optimize            StompOptimizer::optimize              stomp_optimizer.cpp:249-382
 *
 * Floating point: the oracle's contract (-ffp-contract=off, one rounding per operation, every sum
 * sequential in ascending index from 0.0).  tests/CHOMP.md states the operation orders.
 */
#include "../oracle/stomp_oracle.c"

typedef struct {
    double learning_rate;
    double smoothness_cost_weight;
    int use_pseudo_inverse;
    double pseudo_inverse_ridge_factor;
    double field_bias[3];
    const double* joint_update_limits; /* J */
} cr_params;

typedef struct chomp_ref {
    so_problem* P;
    cr_params prm;
    double* upd;       /* J */
    int J, N, Nall, S, nseg;
    double* band;      /* J x Nall x 13: scaled quad_cost_full, entry (r, r - 6 + c) at [r][c] */
    int* joint_seg;    /* J: the segment joint k drives */
    unsigned* seg_mask; /* nseg: joints on the path from the root to the segment (own joint included) */
    double* traj;      /* Nall x J group trajectory */
    double* pos;       /* Nall x S x 3 */
    double *dist, *fgrad, *pot, *pgrad, *vel, *acc, *vmag; /* N x S (x 3) */
    int* col;          /* N x S */
    double *jorg, *jax; /* N x J x 3 */
    double *sinc, *cinc, *finc; /* J x N */
    double* scales;    /* J */
    double* wcost;     /* N */
    double cost;
    int cf;
    int iteration;     /* StompOptimizer::iteration_ of the next step */
    long long n_break, n_skip, n_clamped;
    double* best;      /* J x N */
    frame_t* frames;
} chomp_ref;

/* quad_cost_full_ per joint, scaled by max_cost_scale (stomp_cost.cpp:52-63, 99-104;
 * stomp_optimizer.cpp:105-125), kept as its band: the 7-tap rules squared reach 6 columns */
static int cr_build_quad_full(chomp_ref* c)
{
    const so_problem* P = c->P;
    const int J = c->J, N = c->N, Nall = c->Nall;
    double* Draw = dalloc((size_t)Nall * Nall);
    double* G = dalloc((size_t)Nall * Nall);
    double* Qfull = dalloc((size_t)J * Nall * Nall);
    double* Qfree = dalloc((size_t)N * N);
    double* Qi = dalloc((size_t)N * N);
    double max_scale = 0.0;
    int ok = 1;
    for (int jt = 0; jt < J && ok; ++jt) {
        double* Q = Qfull + (size_t)jt * Nall * Nall;
        double m2 = 1.0;
        for (int d = 0; d < SO_NUM_DIFF_RULES; ++d) {
            m2 *= P->disc;
            memset(Draw, 0, sizeof(double) * (size_t)Nall * Nall);
            for (int i = 0; i < Nall; ++i)
                for (int j = -SO_DIFF_RULE_LENGTH / 2; j <= SO_DIFF_RULE_LENGTH / 2; ++j) {
                    int idx = i + j;
                    if (idx < 0 || idx >= Nall) continue;
                    Draw[(size_t)i * Nall + idx] = DIFF_RULES[d][j + SO_DIFF_RULE_LENGTH / 2];
                }
            gram(Draw, Nall, G);
            double w = P->joints[jt].joint_cost * P->cfg.smoothness_costs[d];
            double f = w * m2;
            for (size_t k = 0; k < (size_t)Nall * Nall; ++k) Q[k] += f * G[k];
        }
        for (int i = 0; i < Nall; ++i) Q[(size_t)i * Nall + i] += 1.0 * P->cfg.ridge_factor;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) Qfree[(size_t)i * N + j] = Q[(size_t)(i + SO_PAD) * Nall + (j + SO_PAD)];
        ok = spd_inverse(Qfree, N, Qi);
        double mx = Qi[0];
        for (size_t k = 1; k < (size_t)N * N; ++k) if (Qi[k] > mx) mx = Qi[k];
        if (max_scale < mx) max_scale = mx;
    }
    if (ok) {
        for (int jt = 0; jt < J; ++jt)
            for (int r = 0; r < Nall; ++r)
                for (int k = 0; k < 13; ++k) {
                    int col = r - 6 + k;
                    double v = 0.0;
                    if (col >= 0 && col < Nall) v = Qfull[((size_t)jt * Nall + r) * Nall + col] * max_scale;
                    c->band[((size_t)jt * Nall + r) * 13 + k] = v;
                }
        /* outside the band the matrix is exactly zero (checked, so that the band is the matrix) */
        for (int jt = 0; jt < J && ok; ++jt)
            for (int r = 0; r < Nall && ok; ++r)
                for (int col = 0; col < Nall; ++col)
                    if ((col < r - 6 || col > r + 6) && Qfull[((size_t)jt * Nall + r) * Nall + col] != 0.0) ok = 0;
    }
    free(Draw); free(G); free(Qfull); free(Qfree); free(Qi);
    return ok;
}

chomp_ref* cr_create(const so_config* cfg, const cr_params* prm)
{
    so_problem* P = so_create(cfg);
    if (!P) return NULL;
    chomp_ref* c = (chomp_ref*)calloc(1, sizeof *c);
    c->P = P;
    c->prm = *prm;
    const int J = c->J = P->J, N = c->N = P->N, Nall = c->Nall = P->Nall, S = c->S = P->S;
    const int nseg = c->nseg = P->nseg;
    const size_t S1 = S ? S : 1;
    c->upd = dup_d(prm->joint_update_limits, J);
    c->prm.joint_update_limits = c->upd;
    c->band = dalloc((size_t)J * Nall * 13);
    c->joint_seg = (int*)calloc((size_t)J, sizeof(int));
    c->seg_mask = (unsigned*)calloc((size_t)nseg, sizeof(unsigned));
    for (int k = 0; k < J; ++k) c->joint_seg[k] = -1;
    for (int s = 0; s < nseg; ++s) {
        const so_segment* sg = &P->segs[s];
        unsigned m = sg->parent >= 0 ? c->seg_mask[sg->parent] : 0u;
        if (sg->q_index >= 0) {
            m |= 1u << sg->q_index;
            if (c->joint_seg[sg->q_index] < 0) c->joint_seg[sg->q_index] = s;
        }
        c->seg_mask[s] = m;
    }
    c->traj = dalloc((size_t)Nall * J);
    c->pos = dalloc((size_t)Nall * S1 * 3);
    c->dist = dalloc((size_t)N * S1); c->pot = dalloc((size_t)N * S1); c->vmag = dalloc((size_t)N * S1);
    c->fgrad = dalloc((size_t)N * S1 * 3); c->pgrad = dalloc((size_t)N * S1 * 3);
    c->vel = dalloc((size_t)N * S1 * 3); c->acc = dalloc((size_t)N * S1 * 3);
    c->col = (int*)calloc((size_t)N * S1, sizeof(int));
    c->jorg = dalloc((size_t)N * J * 3); c->jax = dalloc((size_t)N * J * 3);
    c->sinc = dalloc((size_t)J * N); c->cinc = dalloc((size_t)J * N); c->finc = dalloc((size_t)J * N);
    c->scales = dalloc((size_t)J);
    c->wcost = dalloc((size_t)N);
    c->best = dalloc((size_t)J * N);
    c->frames = (frame_t*)malloc(sizeof(frame_t) * (size_t)nseg);
    if (!cr_build_quad_full(c)) {
        set_err("chomp_ref: quad_cost_full is not banded or not positive definite");
        return NULL;
    }
    return c;
}

void cr_destroy(chomp_ref* c)
{
    if (!c) return;
    so_destroy(c->P);
    free(c->upd); free(c->band); free(c->joint_seg); free(c->seg_mask); free(c->traj); free(c->pos);
    free(c->dist); free(c->pot); free(c->vmag); free(c->fgrad); free(c->pgrad); free(c->vel); free(c->acc);
    free(c->col); free(c->jorg); free(c->jax); free(c->sinc); free(c->cinc); free(c->finc); free(c->scales);
    free(c->wcost); free(c->best); free(c->frames);
    free(c);
}

/* The field's distance and gradient at a point.  The third-party definition: at the
 * nearest cell g, component a is (dist(g + e_a) - dist(g - e_a)) * (1 / (2 res)), with
 * dist = sqrt(double(d2)) * res; a centre whose cell is outside [1, n - 2] on any axis reads
 * distance 0 and gradient 0 (the window of so_sdf_distance, so the neighbours are readable). */
double cr_field_gradient(const chomp_ref* c, double x, double y, double z, double* g)
{
    const so_sdf* f = &c->P->cfg.sdf;
    const double inv = 1.0 / f->resolution;
    double fx = round((x - f->origin[0]) * inv);
    double fy = round((y - f->origin[1]) * inv);
    double fz = round((z - f->origin[2]) * inv);
    g[0] = g[1] = g[2] = 0.0;
    if (!(fx >= 1.0 && fy >= 1.0 && fz >= 1.0 && fx < (double)(f->nx - 1) && fy < (double)(f->ny - 1) &&
          fz < (double)(f->nz - 1)))
        return 0.0;
    const long ix = (long)fx, iy = (long)fy, iz = (long)fz;
    const size_t sx = (size_t)f->ny * f->nz, sy = (size_t)f->nz, at = (size_t)ix * sx + (size_t)iy * sy + (size_t)iz;
    const double res = f->resolution;
    const double inv_twice = 1.0 / (2.0 * res);
#define CR_D(i) (sqrt((double)f->data[i]) * res)
    g[0] = (CR_D(at + sx) - CR_D(at - sx)) * inv_twice;
    g[1] = (CR_D(at + sy) - CR_D(at - sy)) * inv_twice;
    g[2] = (CR_D(at + 1) - CR_D(at - 1)) * inv_twice;
    const double d = CR_D(at);
#undef CR_D
    return d;
}

/* one free waypoint t (0-based in the free block): frames, joint origins and axes, sphere centres,
 * distance, gradient, potential, potential gradient and the collide flags; returns state_is_in_collision_ */
static int cr_fk_one(chomp_ref* c, int t)
{
    const so_problem* P = c->P;
    const int J = c->J, S = c->S;
    double q[SO_MAX_J] = {0.0};
    for (int d = 0; d < J; ++d) q[d] = c->traj[(size_t)(t + SO_PAD) * J + d];
    double* pos = c->pos + (size_t)(t + SO_PAD) * S * 3;
    fk_spheres(P, q, c->frames, pos);
    /* joint origin: the frame's translation (the pose's rotation about the axis leaves it where the
     * parent frame put it); joint axis: the frame's rotation times the stored axis */
    for (int k = 0; k < J; ++k) {
        double* o = c->jorg + ((size_t)t * J + k) * 3;
        double* a = c->jax + ((size_t)t * J + k) * 3;
        o[0] = o[1] = o[2] = a[0] = a[1] = a[2] = 0.0;
        const int sg = c->joint_seg[k];
        if (sg < 0) continue;
        const frame_t* f = &c->frames[sg];
        const double* ax = P->segs[sg].axis;
        for (int i = 0; i < 3; ++i) {
            o[i] = f->p[i];
            a[i] = f->R[3 * i + 0] * ax[0] + f->R[3 * i + 1] * ax[1] + f->R[3 * i + 2] * ax[2];
        }
    }
    int any = 0;
    for (int j = 0; j < S; ++j) {
        const size_t e = (size_t)t * S + j;
        double fg[3];
        const double dist = cr_field_gradient(c, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], fg);
        c->dist[e] = dist;
        for (int i = 0; i < 3; ++i) c->fgrad[3 * e + i] = fg[i];
        for (int i = 0; i < 3; ++i) fg[i] += c->prm.field_bias[i];
        const double r = P->sph[j].radius, cl = P->sph[j].clearance;
        const double d = dist - r;
        double* pg = c->pgrad + 3 * e;
        if (d >= cl) {
            c->pot[e] = 0.0;
            pg[0] = pg[1] = pg[2] = 0.0;
        } else if (d >= 0.0) {
            const double diff = d - cl;
            const double gm = diff * P->inv_clear[j];
            c->pot[e] = 0.5 * gm * diff;
            for (int i = 0; i < 3; ++i) pg[i] = gm * fg[i];
        } else {
            for (int i = 0; i < 3; ++i) pg[i] = fg[i];
            c->pot[e] = -d + 0.5 * cl;
        }
        c->col[e] = dist <= r;
        if (c->col[e]) any = 1;
    }
    return any;
}

/* performForwardKinematics (:618-709) then the cost of doChompOptimization (:233-246).  member is
 * iteration_: at 0 the padding waypoints are part of the pass (their sphere centres are the
 * problem's pad_pos, their collisions its pad_collision). */
static void cr_fk_all(chomp_ref* c, int member)
{
    const so_problem* P = c->P;
    const int N = c->N, S = c->S;
    int cf = !(member == 0 && P->pad_collision);
    memcpy(c->pos, P->pad_pos, sizeof(double) * SO_PAD * S * 3);
    memcpy(c->pos + (size_t)(SO_PAD + N) * S * 3, P->pad_pos + (size_t)SO_PAD * S * 3, sizeof(double) * SO_PAD * S * 3);
    for (int t = 0; t < N; ++t)
        if (cr_fk_one(c, t)) cf = 0;
    const double invTime = 1.0 / P->disc;
    const double invTimeSq = invTime * invTime;
    for (int t = 0; t < N; ++t)
        for (int j = 0; j < S; ++j) {
            const size_t e = (size_t)t * S + j;
            double v[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
            for (int k = -SO_DIFF_RULE_LENGTH / 2; k <= SO_DIFF_RULE_LENGTH / 2; ++k) {
                const double cv = invTime * DIFF_RULES[0][k + SO_DIFF_RULE_LENGTH / 2];
                const double ca = invTimeSq * DIFF_RULES[1][k + SO_DIFF_RULE_LENGTH / 2];
                const double* p = c->pos + ((size_t)(t + SO_PAD + k) * S + j) * 3;
                for (int i = 0; i < 3; ++i) {
                    v[i] += cv * p[i];
                    a[i] += ca * p[i];
                }
            }
            for (int i = 0; i < 3; ++i) {
                c->vel[3 * e + i] = v[i];
                c->acc[3 * e + i] = a[i];
            }
            c->vmag[e] = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
    double cost = 0.0;
    for (int t = 0; t < N; ++t) {
        double state = 0.0, cum = 0.0;
        for (int j = 0; j < S; ++j) {
            cum += c->pot[(size_t)t * S + j] * c->vmag[(size_t)t * S + j];
            state += cum;
        }
        c->wcost[t] = state * P->cfg.obstacle_cost_weight;
        cost += c->wcost[t];
    }
    c->cost = cost;
    c->cf = cf;
}

/* getJacobian of sphere j at free waypoint t: Jm 3 x J row-major */
static void cr_jacobian_at(const chomp_ref* c, int t, int j, double* Jm)
{
    const int J = c->J, S = c->S;
    const unsigned mask = c->seg_mask[c->P->sph[j].segment];
    const double* p = c->pos + ((size_t)(t + SO_PAD) * S + j) * 3;
    for (int k = 0; k < J; ++k) {
        if (!((mask >> k) & 1u)) {
            Jm[0 * J + k] = Jm[1 * J + k] = Jm[2 * J + k] = 0.0;
            continue;
        }
        const double* o = c->jorg + ((size_t)t * J + k) * 3;
        const double* a = c->jax + ((size_t)t * J + k) * 3;
        const double d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
        Jm[0 * J + k] = a[1] * d[2] - a[2] * d[1];
        Jm[1 * J + k] = a[2] * d[0] - a[0] * d[2];
        Jm[2 * J + k] = a[0] * d[1] - a[1] * d[0];
    }
}

static void cr_smoothness(chomp_ref* c)
{
    const int J = c->J, N = c->N, Nall = c->Nall;
    for (int i = 0; i < J; ++i)
        for (int t = 0; t < N; ++t) {
            const int r = t + SO_PAD;
            double s = 0.0;
            for (int k = 0; k < 13; ++k) {
                const int col = r - 6 + k;
                if (col < 0 || col >= Nall) continue;
                s += c->band[((size_t)i * Nall + r) * 13 + k] * (2.0 * c->traj[(size_t)col * J + i]);
            }
            c->sinc[(size_t)i * N + t] = -s;
        }
}

static void cr_collision(chomp_ref* c)
{
    const int J = c->J, N = c->N, S = c->S;
    double Jm[3 * SO_MAX_J];
    for (int t = 0; t < N; ++t) {
        double row[SO_MAX_J];
        for (int k = 0; k < J; ++k) row[k] = 0.0;
        for (int j = 0; j < S; ++j) {
            const size_t e = (size_t)t * S + j;
            const double potential = c->pot[e];
            if (potential <= 1e-10) {
                c->n_skip++;
                continue;
            }
            const double* pg = c->pgrad + 3 * e;
            const double* vel = c->vel + 3 * e;
            const double* acc = c->acc + 3 * e;
            const double vel_mag = c->vmag[e];
            const double vel_mag_sq = vel_mag * vel_mag;
            double nv[3], Pm[9], curv[3], g[3];
            for (int i = 0; i < 3; ++i) nv[i] = vel[i] / vel_mag;   /* a zero vel_mag divides as IEEE says */
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) Pm[3 * r + q] = (r == q ? 1.0 : 0.0) - nv[r] * nv[q];
            for (int r = 0; r < 3; ++r) {
                double pa = 0.0, pgr = 0.0;
                for (int q = 0; q < 3; ++q) pa += Pm[3 * r + q] * acc[q];
                for (int q = 0; q < 3; ++q) pgr += Pm[3 * r + q] * pg[q];
                curv[r] = pa / vel_mag_sq;
                g[r] = vel_mag * (pgr - potential * curv[r]);
            }
            cr_jacobian_at(c, t, j, Jm);
            if (c->prm.use_pseudo_inverse) {
                /* calculatePseudoInverse (:466-470): A = J J^T + ridge I, its inverse by cofactors
                 * over the determinant, pinv = J^T A^-1, row -= pinv g */
                double A[9], C[9], inv[9];
                for (int r = 0; r < 3; ++r)
                    for (int q = 0; q < 3; ++q) {
                        double s = 0.0;
                        for (int k = 0; k < J; ++k) s += Jm[r * J + k] * Jm[q * J + k];
                        A[3 * r + q] = s + (r == q ? 1.0 : 0.0) * c->prm.pseudo_inverse_ridge_factor;
                    }
                C[0] = A[4] * A[8] - A[5] * A[7];
                C[1] = A[5] * A[6] - A[3] * A[8];
                C[2] = A[3] * A[7] - A[4] * A[6];
                C[3] = A[2] * A[7] - A[1] * A[8];
                C[4] = A[0] * A[8] - A[2] * A[6];
                C[5] = A[1] * A[6] - A[0] * A[7];
                C[6] = A[1] * A[5] - A[2] * A[4];
                C[7] = A[2] * A[3] - A[0] * A[5];
                C[8] = A[0] * A[4] - A[1] * A[3];
                const double det = A[0] * C[0] + A[1] * C[1] + A[2] * C[2];
                for (int r = 0; r < 3; ++r)
                    for (int q = 0; q < 3; ++q) inv[3 * r + q] = C[3 * q + r] / det;
                for (int k = 0; k < J; ++k) {
                    double s = 0.0;
                    for (int q = 0; q < 3; ++q) {
                        double pk = 0.0;
                        for (int r = 0; r < 3; ++r) pk += Jm[r * J + k] * inv[3 * r + q];
                        s += pk * g[q];
                    }
                    row[k] -= s;
                }
            } else {
                for (int k = 0; k < J; ++k) {
                    double s = 0.0;
                    for (int r = 0; r < 3; ++r) s += Jm[r * J + k] * g[r];
                    row[k] -= s;
                }
            }
            if (c->col[e]) {
                c->n_break++;
                break;
            }
        }
        for (int k = 0; k < J; ++k) c->cinc[(size_t)k * N + t] = row[k];
    }
}

static void cr_total(chomp_ref* c)
{
    const int J = c->J, N = c->N;
    const double ws = c->prm.smoothness_cost_weight, wo = c->P->cfg.obstacle_cost_weight;
    double rhs[4096];
    for (int i = 0; i < J; ++i) {
        const double* Qi = c->P->Qinv + (size_t)i * N * N;
        for (int k = 0; k < N; ++k) rhs[k] = ws * c->sinc[(size_t)i * N + k] + wo * c->cinc[(size_t)i * N + k];
        for (int r = 0; r < N; ++r) {
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += Qi[(size_t)r * N + k] * rhs[k];
            c->finc[(size_t)i * N + r] = c->prm.learning_rate * s;
        }
    }
}

static void cr_add(chomp_ref* c)
{
    const int J = c->J, N = c->N;
    for (int i = 0; i < J; ++i) {
        const double* f = c->finc + (size_t)i * N;
        double scale = 1.0;
        double max = f[0], min = f[0];
        for (int k = 1; k < N; ++k) {
            if (f[k] > max) max = f[k];
            if (f[k] < min) min = f[k];
        }
        const double max_scale = c->prm.joint_update_limits[i] / fabs(max);
        const double min_scale = c->prm.joint_update_limits[i] / fabs(min);
        if (max_scale < scale) scale = max_scale;
        if (min_scale < scale) scale = min_scale;
        c->scales[i] = scale;
        for (int k = 0; k < N; ++k) c->traj[(size_t)(k + SO_PAD) * J + i] += scale * f[k];
    }
}

static void cr_limits(chomp_ref* c)
{
    const size_t n = (size_t)c->Nall * c->J;
    double* before = (double*)malloc(sizeof(double) * n);
    memcpy(before, c->traj, sizeof(double) * n);
    handle_joint_limits(c->P, c->traj);
    if (memcmp(before, c->traj, sizeof(double) * n)) c->n_clamped++;
    free(before);
}

/* optimize()'s pass before the loop (:267-271): the policy into the group trajectory, the joint
 * limits, FK of every waypoint (iteration_ = 0).  traj: J x N or NULL (theta_0). */
int cr_reset(chomp_ref* c, const double* traj)
{
    const so_problem* P = c->P;
    const int J = c->J, N = c->N, Nall = c->Nall;
    if (N > 4096) return -1;
    const double* src = traj ? traj : P->theta;
    for (int i = 0; i < Nall; ++i)
        for (int d = 0; d < J; ++d) {
            double v;
            if (i < SO_PAD) v = P->cfg.start[d];
            else if (i >= SO_PAD + N) v = P->cfg.goal[d];
            else v = src[(size_t)d * N + (i - SO_PAD)];
            c->traj[(size_t)i * J + d] = v;
        }
    memset(c->sinc, 0, sizeof(double) * (size_t)J * N);
    memset(c->cinc, 0, sizeof(double) * (size_t)J * N);
    memset(c->finc, 0, sizeof(double) * (size_t)J * N);
    memset(c->scales, 0, sizeof(double) * (size_t)J);
    c->iteration = 0;
    c->n_break = c->n_skip = c->n_clamped = 0;
    cr_limits(c);
    cr_fk_all(c, 0);
    return 0;
}

static void cr_step_one(chomp_ref* c)
{
    cr_smoothness(c);
    cr_collision(c);
    cr_total(c);
    cr_add(c);
    cr_limits(c);
    cr_fk_all(c, c->iteration);
    c->iteration++;
}

int cr_step(chomp_ref* c, int count)
{
    for (int i = 0; i < count; ++i) cr_step_one(c);
    return 0;
}

static void cr_free_block(const chomp_ref* c, double* out)
{
    for (int d = 0; d < c->J; ++d)
        for (int i = 0; i < c->N; ++i) out[(size_t)d * c->N + i] = c->traj[(size_t)(i + SO_PAD) * c->J + d];
}

/* the loop of optimize() with doChompOptimization (:284-359), from the state cr_reset left;
 * last_trajectory_constraints_satisfied_ is true (:231) */
int cr_optimize(chomp_ref* c, so_stats* st, double* costs_per_it, double* best)
{
    so_stats s;
    s.collision_success_iteration = -1;
    s.success_iteration = -1;
    s.success = 0;
    s.last_improvement_iteration = -1;
    int cfi = 0;
    double best_cost = 0.0;
    int it;
    for (it = 0; it < c->P->cfg.max_iterations; it++) {
        cr_step_one(c);
        const int ok = c->cf;
        if (ok) cfi++;
        else cfi = 0;
        if (c->cf && s.collision_success_iteration == -1) s.collision_success_iteration = it;
        if (ok && s.success_iteration == -1) {
            s.success_iteration = it;
            s.success = 1;
        }
        const double cost = c->cost;
        if (costs_per_it) costs_per_it[it] = cost;
        if (it == 0) {
            cr_free_block(c, c->best);
            best_cost = cost;
        } else if (cost < best_cost && ok) {
            cr_free_block(c, c->best);
            best_cost = cost;
            s.last_improvement_iteration = it;
        }
        if (cfi >= c->P->cfg.max_iterations_after_collision_free) {
            it++;
            break;
        }
    }
    s.iterations = it;
    s.best_cost = best_cost;
    if (st) *st = s;
    if (best) memcpy(best, c->best, sizeof(double) * (size_t)c->J * c->N);
    return 0;
}

/* the intermediates, named and shaped as stomp_chomp_get's for one descent; returns the number of
 * doubles written, -1 for an unknown name */
long long cr_get(const chomp_ref* c, const char* which, double* out)
{
    const size_t J = c->J, N = c->N, S = c->S, Nall = c->Nall;
    size_t n = 0;
    const double* src = NULL;
    if (!strcmp(which, "trajectory")) { cr_free_block(c, out); return (long long)(J * N); }
    else if (!strcmp(which, "smoothness_increments")) { src = c->sinc; n = J * N; }
    else if (!strcmp(which, "collision_increments")) { src = c->cinc; n = J * N; }
    else if (!strcmp(which, "final_increments")) { src = c->finc; n = J * N; }
    else if (!strcmp(which, "scales")) { src = c->scales; n = J; }
    else if (!strcmp(which, "sphere_positions")) { src = c->pos; n = Nall * S * 3; }
    else if (!strcmp(which, "distances")) { src = c->dist; n = N * S; }
    else if (!strcmp(which, "field_gradients")) { src = c->fgrad; n = N * S * 3; }
    else if (!strcmp(which, "potentials")) { src = c->pot; n = N * S; }
    else if (!strcmp(which, "potential_gradients")) { src = c->pgrad; n = N * S * 3; }
    else if (!strcmp(which, "velocities")) { src = c->vel; n = N * S * 3; }
    else if (!strcmp(which, "accelerations")) { src = c->acc; n = N * S * 3; }
    else if (!strcmp(which, "vel_mags")) { src = c->vmag; n = N * S; }
    else if (!strcmp(which, "joint_origins")) { src = c->jorg; n = N * J * 3; }
    else if (!strcmp(which, "joint_axes")) { src = c->jax; n = N * J * 3; }
    else if (!strcmp(which, "costs")) { src = c->wcost; n = N; }
    else if (!strcmp(which, "cost")) { out[0] = c->cost; return 1; }
    else if (!strcmp(which, "collision_free")) { out[0] = c->cf ? 1.0 : 0.0; return 1; }
    else return -1;
    memcpy(out, src, sizeof(double) * n);
    return (long long)n;
}

/* how often the break after a colliding sphere and the 1e-10 skip fired, and how many limit passes
 * changed the trajectory, since cr_reset */
void cr_counts(const chomp_ref* c, long long* out)
{
    out[0] = c->n_break;
    out[1] = c->n_skip;
    out[2] = c->n_clamped;
}

/* the Jacobian (3 x J row-major) of sphere j at the joint vector q: one waypoint evaluated in
 * place of free waypoint 0 (the caller resets afterwards) */
int cr_jacobian(chomp_ref* c, const double* q, int j, double* Jm)
{
    if (j < 0 || j >= c->S) return -1;
    for (int d = 0; d < c->J; ++d) c->traj[(size_t)SO_PAD * c->J + d] = q[d];
    cr_fk_one(c, 0);
    cr_jacobian_at(c, 0, j, Jm);
    return 0;
}

int cr_sphere_positions(const chomp_ref* c, const double* q, double* out)
{
    return so_sphere_positions(c->P, q, out);
}

int cr_theta(const chomp_ref* c, double* out) { return so_get_theta(c->P, out); }
int cr_pad_collision(const chomp_ref* c) { return c->P->pad_collision; }
