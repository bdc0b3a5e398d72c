/*
 * ss_graph.hip -- essential-graph optimisation: the Sim3 pose graph of Optimizer::OptimizeEssentialGraph for every loop (problem) of
 * a call at once, and the map-point correction that follows it (the rule: include/sendslam_orb.h; DESIGN.md "Essential-graph
 * optimisation").  Every step of the arithmetic is the text of ss_graph_steps.h, which the host twin compiles too.
 *
 * The host enqueues the fixed schedule of every step without a round trip; a problem's state (ssk_graph_state) lives in device
 * memory, and a kernel whose problem has ended returns at once.
 *
 *   G-A  k_graph_gather_kf, k_graph_gather_edges, k_graph_gather_state   the start into both buffers and its usable bytes, M_e per
 *                         edge, the problem's state
 *   G-B  k_graph_lin      sixteen lanes per edge over (edges, problems): lane c < 14 one perturbed column (two error evaluations),
 *                         lane 14 the error; e and the 7 x 14 block go to the workspace
 *   G-C  k_graph_blocks   one lane per keyframe over (keyframes, problems): H_vv, g_v, the damping terms, the factor of the block
 *   G-D  k_graph_solve    one workgroup per problem: the whole PCG loop on vectors in the workspace, its dot products by
 *                         gn_block_sum, then the trial Sim3s into the other buffer
 *   G-E  k_graph_cost     one workgroup per problem: that workgroup is the tree of the cost; its thread 0 then accepts or rejects
 *   G-F  k_graph_finish   the outputs
 *        k_graph_points   the map-point correction
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store; there are
 * no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_gn.h"
#include "ss_graph_steps.h"
#include "ss_kernels.h"

namespace {

static_assert(SS_GN_SLOTS == 256, "four waves, one group of 64 slots each");
static_assert(sizeof(ss_graph_result) == 48 && sizeof(ss_graph_params) == 48 && sizeof(ss_graph_problem) == 16, "the layouts of the header");

#define GRAPH_LANES 16                         /* lanes of an edge in k_graph_lin */
#define GRAPH_EDGES_PER_BLOCK (SS_GN_SLOTS / GRAPH_LANES)
#define GRAPH_BLOCK_LANES 64                   /* keyframes of a workgroup of k_graph_blocks */

struct graph_prob {
    int k0, n_kf, e0, n_edges;
};

/* the host has checked the table: the clamps only keep a stray value inside the arrays */
__device__ __forceinline__ graph_prob graph_prob_of(const ssk_graph_call &a, int q)
{
    const ss_graph_problem p = a.prob[q];
    graph_prob r;
    r.n_kf = min(max(p.n_kf, 1), a.n_kf);
    r.k0 = min(max(p.first_kf, 0), a.n_kf - r.n_kf);
    r.n_edges = min(max(p.n_edges, 0), a.n_edges);
    r.e0 = min(max(p.first_edge, 0), a.n_edges - r.n_edges);
    return r;
}

__device__ __forceinline__ double *graph_S(const ssk_graph_call &a, int buf, int v) { return a.S + ((size_t)buf * a.n_kf + v) * SS_GRAPH_SIM3; }

/* an endpoint of edge e, kept inside the problem */
__device__ __forceinline__ int graph_end(const ssk_graph_call &a, const graph_prob &pr, int e, int side)
{
    return min(max(a.edges[2 * (size_t)e + side], pr.k0), pr.k0 + pr.n_kf - 1);
}

__device__ __forceinline__ void graph_load(const double *src, double *dst)
{
#pragma unroll
    for (int k = 0; k < SS_GRAPH_SIM3; k++) dst[k] = src[k];
}

/* G-A.  grid (keyframes / 256): every keyframe of the call */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_gather_kf(ssk_graph_call a)
{
    const int v = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (v >= a.n_kf) return;
    double S[SS_GRAPH_SIM3], N[SS_GRAPH_SIM3];
    graph_load(a.start + (size_t)v * SS_GRAPH_SIM3, S);
    graph_load(a.nc + (size_t)v * SS_GRAPH_SIM3, N);
#pragma unroll
    for (int k = 0; k < SS_GRAPH_SIM3; k++) graph_S(a, 0, v)[k] = S[k], graph_S(a, 1, v)[k] = S[k];
    a.flag[v] = ss_graph_usable(S) && ss_graph_usable(N) ? 1 : 0;
}

/* grid (max_edges / 256, problems) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_gather_edges(ssk_graph_call a)
{
    const int q = (int)blockIdx.y, le = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    const graph_prob pr = graph_prob_of(a, q);
    if (le >= pr.n_edges) return;
    const int e = pr.e0 + le;
    double Ni[SS_GRAPH_SIM3], Nj[SS_GRAPH_SIM3], M[SS_GRAPH_SIM3];
    graph_load(a.nc + (size_t)graph_end(a, pr, e, 0) * SS_GRAPH_SIM3, Ni);
    graph_load(a.nc + (size_t)graph_end(a, pr, e, 1) * SS_GRAPH_SIM3, Nj);
    ss_graph_measure(Ni, Nj, M);
#pragma unroll
    for (int k = 0; k < SS_GRAPH_SIM3; k++) a.M[(size_t)e * SS_GRAPH_SIM3 + k] = M[k];
}

/* grid (problems) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_gather_state(ssk_graph_call a)
{
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    const graph_prob pr = graph_prob_of(a, q);
    int n_free = 0, n_bad = 0, buf = 0;
    for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) n_free += a.fixed[pr.k0 + v] ? 0 : 1, n_bad += a.flag[pr.k0 + v] ? 0 : 1;
    n_free = gn_block_sum(n_free, part_n, &buf);
    n_bad = gn_block_sum(n_bad, part_n, &buf);
    if (tid != 0) return;
    ssk_graph_state s;
    s.lambda = a.p.lambda, s.cost0 = 0.0, s.cost_before = 0.0;
    s.state = n_bad > 0 ? 2 : (n_free == 0 || pr.n_edges == 0) ? 1 : 0;
    s.ended = s.state != 0 ? 1 : 0;
    s.cur = 0, s.n_free = n_free, s.steps = 0, s.accepted = 0, s.pcg = 0, s.trial_finite = 0;
    a.st[q] = s;
}

/* G-B.  grid (max_edges / 16, problems) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_lin(ssk_graph_call a)
{
    const int q = (int)blockIdx.y, lane = (int)threadIdx.x % GRAPH_LANES;
    const int le = (int)blockIdx.x * GRAPH_EDGES_PER_BLOCK + (int)threadIdx.x / GRAPH_LANES;
    if (a.st[q].ended != 0) return; /* uniform */
    const graph_prob pr = graph_prob_of(a, q);
    if (le >= pr.n_edges || lane == GRAPH_LANES - 1) return;
    const int e = pr.e0 + le, cur = a.st[q].cur & 1;
    const int i = graph_end(a, pr, e, 0), j = graph_end(a, pr, e, 1);
    const bool fix = a.p.fix_scale != 0;
    double M[SS_GRAPH_SIM3], Si[SS_GRAPH_SIM3], Sj[SS_GRAPH_SIM3], out[7];
    graph_load(a.M + (size_t)e * SS_GRAPH_SIM3, M);
    graph_load(graph_S(a, cur, i), Si);
    graph_load(graph_S(a, cur, j), Sj);
    if (lane == 14) {
        ss_graph_error(M, Si, Sj, out);
#pragma unroll
        for (int r = 0; r < 7; r++) a.err[(size_t)e * 7 + r] = out[r];
        return;
    }
    const int side = lane / 7, c = lane % 7;
    ss_graph_column(M, Si, Sj, side, c, fix, a.fixed[side ? j : i] != 0 || (fix && c == 6), out);
#pragma unroll
    for (int r = 0; r < 7; r++) a.J[((size_t)e * 14 + lane) * 7 + r] = out[r];
}

/* G-C.  grid (max_kf / 64, problems) */
__global__ __launch_bounds__(GRAPH_BLOCK_LANES) void k_graph_blocks(ssk_graph_call a)
{
    const int q = (int)blockIdx.y, lv = (int)blockIdx.x * GRAPH_BLOCK_LANES + (int)threadIdx.x;
    if (a.st[q].ended != 0) return; /* uniform */
    const graph_prob pr = graph_prob_of(a, q);
    if (lv >= pr.n_kf) return;
    const int v = pr.k0 + lv;
    if (a.fixed[v]) {
#pragma unroll
        for (int k = 0; k < 7; k++) a.dd[(size_t)v * 7 + k] = 0.0, a.g[(size_t)v * 7 + k] = 0.0;
        a.flag[v] = 1;
        return;
    }
    /* the run of inc, kept inside the array */
    const int off = min(max(a.inc_off[v], 0), 2 * a.n_edges), cnt = min(max(a.inc_cnt[v], 0), 2 * a.n_edges - off);
    const bool ok = ss_graph_vertex_block(a.inc + off, cnt, a.J, a.err, a.p.fix_scale != 0 ? 6 : 7, a.st[q].lambda, a.L + (size_t)v * 49, a.dd + (size_t)v * 7,
                                          a.g + (size_t)v * 7);
    a.flag[v] = ok ? 1 : 0;
}

/* the tree of a dot product over the 7 n_kf entries of a problem: thread s is slot s */
__device__ __forceinline__ double graph_dot(const double *x, const double *y, int n, double (*part)[4][1], int *buf)
{
    double sum[1] = {0.0};
    for (int k = (int)threadIdx.x; k < n; k += SS_GN_SLOTS) sum[0] = sum[0] + x[k] * y[k];
    gn_block_sum(sum, part, buf);
    return sum[0];
}

/* G-D.  grid (problems).  The vectors of the solve are the problem's rows of the workspace arrays; a thread owns the keyframes tid,
 * tid + 256, ... in the keyframe-wise phases and the edges tid, tid + 256, ... in the edge-wise one; a barrier stands between two
 * phases whenever the second reads what other threads wrote in the first */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_solve(ssk_graph_call a)
{
    __shared__ double part[2][4][1];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (a.st[q].ended != 0) return; /* uniform */
    const graph_prob pr = graph_prob_of(a, q);
    const int n = a.p.fix_scale != 0 ? 6 : 7, cur = a.st[q].cur & 1, n7 = 7 * pr.n_kf;
    const bool fix = a.p.fix_scale != 0;
    const size_t base = (size_t)pr.k0 * 7;
    double *x = a.x + base, *r = a.r + base, *z = a.z + base, *p = a.pv + base, *qv = a.q + base;
    const double *g = a.g + base, *dd = a.dd + base;
    int bad = 0, buf = 0;
    for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) bad |= a.flag[pr.k0 + v] ? 0 : 1;
    if (__syncthreads_or(bad)) {
        if (tid == 0) a.st[q].state = 2, a.st[q].ended = 1;
        return;
    }
    auto precondition = [&](int v) {
#pragma unroll
        for (int k = 0; k < 7; k++) z[(size_t)v * 7 + k] = r[(size_t)v * 7 + k];
        if (!a.fixed[pr.k0 + v]) ss_gn_subst_n(a.L + (size_t)(pr.k0 + v) * 49, n, 7, z + (size_t)v * 7);
    };
    for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
        const bool free_v = a.fixed[pr.k0 + v] == 0;
#pragma unroll
        for (int k = 0; k < 7; k++) x[(size_t)v * 7 + k] = 0.0, r[(size_t)v * 7 + k] = (free_v && k < n) ? -g[(size_t)v * 7 + k] : 0.0;
        precondition(v);
#pragma unroll
        for (int k = 0; k < 7; k++) p[(size_t)v * 7 + k] = z[(size_t)v * 7 + k];
    }
    __syncthreads();
    double rho = graph_dot(r, z, n7, part, &buf);
    const double stop = (a.p.pcg_tol * a.p.pcg_tol) * rho;
    int done = 0;
    while (done < a.p.pcg_iterations) { /* every exit is uniform: the scalars come out of the trees */
        for (int le = tid; le < pr.n_edges; le += SS_GN_SLOTS) {
            const int e = pr.e0 + le;
            double u[7];
            ss_graph_edge_product(a.J + (size_t)e * 98, a.pv + (size_t)graph_end(a, pr, e, 0) * 7, a.pv + (size_t)graph_end(a, pr, e, 1) * 7, u);
#pragma unroll
            for (int k = 0; k < 7; k++) a.u[(size_t)e * 7 + k] = u[k];
        }
        __syncthreads();
        for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
            const int gv = pr.k0 + v;
            if (a.fixed[gv]) {
#pragma unroll
                for (int k = 0; k < 7; k++) qv[(size_t)v * 7 + k] = 0.0;
                continue;
            }
            const int off = min(max(a.inc_off[gv], 0), 2 * a.n_edges), cnt = min(max(a.inc_cnt[gv], 0), 2 * a.n_edges - off);
            ss_graph_vertex_product(a.inc + off, cnt, a.J, a.u, n, dd + (size_t)v * 7, p + (size_t)v * 7, qv + (size_t)v * 7);
        }
        __syncthreads();
        const double pq = graph_dot(p, qv, n7, part, &buf);
        if (!(pq > 0.0)) break;
        const double alpha = rho / pq;
        for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const size_t o = (size_t)v * 7 + k;
                x[o] = x[o] + alpha * p[o], r[o] = r[o] - alpha * qv[o];
            }
            precondition(v);
        }
        done++;
        __syncthreads();
        const double rho1 = graph_dot(r, z, n7, part, &buf);
        if (rho1 <= stop) break;
        const double beta = rho1 / rho;
        for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
#pragma unroll
            for (int k = 0; k < 7; k++) p[(size_t)v * 7 + k] = z[(size_t)v * 7 + k] + beta * p[(size_t)v * 7 + k];
        }
        rho = rho1;
        __syncthreads();
    }
    /* the trial Sim3s of every keyframe of the problem into the other buffer: a thread reads its own rows of x */
    bool large = false, finite = true;
    for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
        double T[SS_GRAPH_SIM3], d[7];
        graph_load(graph_S(a, cur, pr.k0 + v), T);
#pragma unroll
        for (int k = 0; k < 7; k++) d[k] = x[(size_t)v * 7 + k];
        if (!a.fixed[pr.k0 + v] && !ss_graph_retract(d, fix, T)) large = true;
#pragma unroll
        for (int k = 0; k < SS_GRAPH_SIM3; k++) finite = finite && ss_gn_is_finite(T[k]), graph_S(a, cur ^ 1, pr.k0 + v)[k] = T[k];
    }
    const int any_large = __syncthreads_or(large ? 1 : 0);
    const int all_finite = __syncthreads_and(finite ? 1 : 0);
    if (tid != 0) return;
    a.st[q].pcg = a.st[q].pcg + done;
    if (any_large) a.st[q].state = 4, a.st[q].ended = 1;
    a.st[q].trial_finite = all_finite;
}

/* G-E.  grid (problems): the cost of the current (begin) or the trial state, then the decision */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_cost(ssk_graph_call a, int begin)
{
    __shared__ double part[2][4][1];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (a.st[q].ended != 0) return; /* uniform */
    const graph_prob pr = graph_prob_of(a, q);
    const int buf_state = (a.st[q].cur & 1) ^ (begin ? 0 : 1);
    double sum[1] = {0.0};
    for (int le = tid; le < pr.n_edges; le += SS_GN_SLOTS) {
        const int e = pr.e0 + le;
        double M[SS_GRAPH_SIM3], Si[SS_GRAPH_SIM3], Sj[SS_GRAPH_SIM3];
        graph_load(a.M + (size_t)e * SS_GRAPH_SIM3, M);
        graph_load(graph_S(a, buf_state, graph_end(a, pr, e, 0)), Si);
        graph_load(graph_S(a, buf_state, graph_end(a, pr, e, 1)), Sj);
        sum[0] = sum[0] + ss_graph_cost_term(M, Si, Sj);
    }
    int buf = 0;
    gn_block_sum(sum, part, &buf); /* its barrier stands between every thread's reads of the state and thread 0's writes */
    if (tid != 0) return;
    ssk_graph_state *s = a.st + q;
    const double cost = sum[0];
    if (begin) {
        if (!ss_gn_is_finite(cost)) {
            s->state = 2, s->ended = 1;
            return;
        }
        s->cost0 = cost, s->cost_before = cost;
        return;
    }
    const bool accepted = s->trial_finite != 0 && ss_gn_is_finite(cost) && cost <= s->cost0;
    s->steps = s->steps + 1;
    s->lambda = ss_ba_next_lambda(s->lambda, accepted, a.p.lambda_factor, a.p.lambda_min);
    if (!accepted) return;
    s->accepted = s->accepted + 1;
    s->cost0 = cost;
    s->cur = s->cur ^ 1;
}

/* G-F.  grid (max(keyframes, problems) / 256): every keyframe's Sim3 and pose; thread q < n_problems writes problem q's result */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_finish(ssk_graph_call a)
{
    const int v = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (v < a.n_kf) {
        const int q = a.kf_prob[v];
        const int buf = (q >= 0 && q < a.n_problems) ? (a.st[q].cur & 1) : 0;
        double S[SS_GRAPH_SIM3], pose[12];
        graph_load(graph_S(a, buf, v), S);
        ss_graph_pose(S, pose);
#pragma unroll
        for (int k = 0; k < SS_GRAPH_SIM3; k++) a.out_sim3[(size_t)v * SS_GRAPH_SIM3 + k] = S[k];
#pragma unroll
        for (int k = 0; k < 12; k++) a.out_pose[(size_t)v * 12 + k] = pose[k];
    }
    if (v >= a.n_problems) return;
    const ssk_graph_state s = a.st[v];
    ss_graph_result r;
    r.lambda = s.lambda, r.cost_before = s.cost_before, r.cost_after = s.cost0;
    r.state = s.state, r.n_edges = graph_prob_of(a, v).n_edges, r.n_free = s.n_free;
    r.steps = s.steps, r.accepted = s.accepted, r.pcg_iterations = s.pcg;
    a.result[v] = r;
}

/* grid (point_rows / 256, blocks) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_graph_points(ssk_graph_points_call a)
{
    const int b = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (i >= a.point_rows) return;
    const size_t o = (size_t)b * a.point_rows + i;
    const int r = a.ref[o];
    if (r < 0 || r >= a.n_kf) return;
    double N[SS_GRAPH_SIM3], S[SS_GRAPH_SIM3];
    graph_load(a.nc + (size_t)r * SS_GRAPH_SIM3, N);
    graph_load(a.sim3 + (size_t)r * SS_GRAPH_SIM3, S);
    ss_map_point *p = a.points + o;
    double x[3] = {(double)p->x, (double)p->y, (double)p->z};
    ss_graph_point(N, S, x);
    p->x = (float)x[0], p->y = (float)x[1], p->z = (float)x[2];
}

inline unsigned blocks_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

} // namespace

void ssk_graph_gather(hipStream_t s, const ssk_graph_call &g)
{
    hipLaunchKernelGGL(k_graph_gather_kf, dim3(blocks_of(g.n_kf, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
    if (g.n_problems == 0) return;
    if (g.max_edges > 0) hipLaunchKernelGGL(k_graph_gather_edges, dim3(blocks_of(g.max_edges, SS_GN_SLOTS), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_graph_gather_state, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_graph_lin(hipStream_t s, const ssk_graph_call &g)
{
    if (g.max_edges == 0) return; /* no problem of the call runs */
    hipLaunchKernelGGL(k_graph_lin, dim3(blocks_of(g.max_edges, GRAPH_EDGES_PER_BLOCK), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_graph_blocks(hipStream_t s, const ssk_graph_call &g)
{
    hipLaunchKernelGGL(k_graph_blocks, dim3(blocks_of(g.max_kf, GRAPH_BLOCK_LANES), (unsigned)g.n_problems), dim3(GRAPH_BLOCK_LANES), 0, s, g);
}

void ssk_graph_solve(hipStream_t s, const ssk_graph_call &g) { hipLaunchKernelGGL(k_graph_solve, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g); }

void ssk_graph_cost(hipStream_t s, const ssk_graph_call &g, int begin)
{
    hipLaunchKernelGGL(k_graph_cost, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g, begin);
}

void ssk_graph_finish(hipStream_t s, const ssk_graph_call &g)
{
    hipLaunchKernelGGL(k_graph_finish, dim3(blocks_of(g.n_kf > g.n_problems ? g.n_kf : g.n_problems, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_graph_points(hipStream_t s, const ssk_graph_points_call &g)
{
    hipLaunchKernelGGL(k_graph_points, dim3(blocks_of(g.point_rows, SS_GN_SLOTS), (unsigned)g.n_blocks), dim3(SS_GN_SLOTS), 0, s, g);
}
