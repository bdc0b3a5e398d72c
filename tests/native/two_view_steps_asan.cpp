/* The steps of the two-view initialisation (csrc/ss_two_view_steps.h, the text the kernels and the host twins compile) as a
 * stand-alone program for -fsanitize=address,undefined: the draws over several counts, the model on 20 000 ordinary, degenerate and
 * non-finite octuples, the decompositions and CheckRT on what they give, and one whole problem of 300 correspondences the way the
 * kernels run it.  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_two_view_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static const ss_tv_cam CAM = {500.0, 510.0, 318.0, 243.0};
static const double R21[9] = {0.99870032, -0.00998734, -0.04997917, 0.00899837, 0.99976001, -0.01997367, 0.05016666, 0.01949798, 0.99855052};
static const double T21[3] = {0.6, 0.1, 0.9};

/* a point in front of camera 1 seen by both cameras */
static void observe(uint32_t &s, bool planar, float noise, float uv[4])
{
    double z = 4.0 + 4.0 * unit(s);
    const double x = (unit(s) - 0.5) * 0.9 * z, y = (unit(s) - 0.5) * 0.6 * z;
    if (planar) z = 6.0 + 0.3 * x - 0.2 * y;
    const double X2[3] = {R21[0] * x + R21[1] * y + R21[2] * z + T21[0], R21[3] * x + R21[4] * y + R21[5] * z + T21[1],
                          R21[6] * x + R21[7] * y + R21[8] * z + T21[2]};
    uv[0] = (float)(CAM.fx * x / z + CAM.cx) + noise * (unit(s) - 0.5f), uv[1] = (float)(CAM.fy * y / z + CAM.cy) + noise * (unit(s) - 0.5f);
    uv[2] = (float)(CAM.fx * X2[0] / X2[2] + CAM.cx) + noise * (unit(s) - 0.5f), uv[3] = (float)(CAM.fy * X2[1] / X2[2] + CAM.cy) + noise * (unit(s) - 0.5f);
}

int main()
{
    long steps = 0;
    uint32_t s = 8642u;
    /* the draws: distinct, in range, a permutation at n = 8 */
    const int counts[] = {8, 9, 10, 64, 65, 1000, 16384};
    for (int n : counts) {
        for (int t = 0; t < 1024; t++) {
            int p[SS_TV_DRAWS];
            ss_tv_draw(lcg(s), (uint32_t)(t & 7), t, n, p);
            for (int k = 0; k < SS_TV_DRAWS; k++) {
                if (p[k] < 0 || p[k] >= n) return printf("draw out of range: n %d t %d\n", n, t), 1;
                for (int e = 0; e < k; e++)
                    if (p[e] == p[k]) return printf("draw repeats: n %d t %d\n", n, t), 1;
            }
            steps++;
        }
    }
    /* the model: random, planar, collinear, identical, repeated, huge, NaN and infinite octuples; every entry of a model is finite,
     * a zero model is all 0.0 */
    const float odd[] = {0.0f, -0.0f, 1e-45f, 3e38f, -3e38f, 1e30f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    long zero_h = 0, zero_f = 0, hyps = 0;
    for (int it = 0; it < 20000; it++) {
        float uv[4 * SS_TV_DRAWS];
        int pick[SS_TV_DRAWS];
        for (int k = 0; k < SS_TV_DRAWS; k++) observe(s, it % 9 == 1, it % 2 ? 1.0f : 0.0f, uv + 4 * k), pick[k] = 3 * k;
        if (it % 9 == 2)
            for (int k = 1; k < SS_TV_DRAWS; k++)
                for (int c = 0; c < 4; c++) uv[4 * k + c] = uv[c] + (float)k * (c & 1 ? 3.0f : 7.0f); /* collinear in both images */
        if (it % 9 == 3)
            for (int k = 4; k < 4 * SS_TV_DRAWS; k++) uv[k] = uv[k % 4]; /* identical */
        if (it % 9 == 4) pick[5] = pick[2];
        if (it % 9 == 5) uv[lcg(s) % 32] = odd[lcg(s) % 8], uv[lcg(s) % 32] = odd[lcg(s) % 8];
        if (it % 9 == 6)
            for (int c = 0; c < 4; c++) uv[4 + c] = uv[c]; /* a repeated row */
        if (it % 9 == 7)
            for (int k = 0; k < SS_TV_DRAWS; k++) uv[4 * k + 2] = uv[4 * k], uv[4 * k + 3] = uv[4 * k + 1]; /* no motion */
        const ss_tv_norm nm = ss_tv_normalise_host(uv, SS_TV_DRAWS);
        if (!ss_tv_norm_ok(nm)) {
            steps++;
            continue;
        }
        ss_tv_work_host w;
        ss_tv_model m;
        ss_tv_model_of(uv, pick, nm, w, m);
        for (int k = 0; k < 9; k++) {
            if (!std::isfinite(m.h21[k]) || !std::isfinite(m.h12[k]) || !std::isfinite(m.f21[k])) return printf("a model entry is not finite\n"), 1;
            if (!m.ok_h && (m.h21[k] != 0.0 || m.h12[k] != 0.0)) return printf("a zero H is not zero\n"), 1;
            if (!m.ok_f && m.f21[k] != 0.0) return printf("a zero F is not zero\n"), 1;
        }
        if (it % 9 == 4 && (m.ok_h || m.ok_f)) return printf("a repeated draw gave a model\n"), 1;
        zero_h += m.ok_h ? 0 : 1, zero_f += m.ok_f ? 0 : 1;
        /* the decompositions of whatever came out, and CheckRT of the eight under each hypothesis */
        double hyp[12 * SS_TV_MAX_HYP];
        for (int branch = 0; branch < 2; branch++) {
            if (!(branch ? m.ok_h : m.ok_f)) continue;
            const int n_hyp = branch ? ss_tv_decompose_h(m.h21, CAM, hyp) : ss_tv_decompose_f(m.f21, CAM, hyp);
            for (int h = 0; h < n_hyp; h++)
                for (int k = 0; k < SS_TV_DRAWS; k++) {
                    ss_tv_point q;
                    if (ss_tv_check_rt(hyp + 12 * h, hyp + 12 * h + 9, CAM, uv[4 * k], uv[4 * k + 1], uv[4 * k + 2], uv[4 * k + 3], &q)) {
                        const ss_map_point mp = ss_tv_map_point(q, 1.2f, 2.0736f);
                        if (!std::isfinite(mp.x) || !std::isfinite(mp.max_dist)) return printf("a good point is not finite\n"), 1;
                    }
                    hyps++;
                }
        }
        steps++;
    }
    if (zero_h == 0 || zero_f == 0 || zero_h > 15000) return printf("zero models: %ld H, %ld F of 20000\n", zero_h, zero_f), 1;
    /* a whole problem: 300 correspondences, 30 % gross outliers, a few odd numbers, on exact-size arrays */
    const int n = 300;
    ss_two_view_params p = {};
    p.chi2_h = 5.991, p.chi2_f = 3.841, p.chi2_score = 5.991, p.rh_threshold = 0.45, p.cos_min_parallax = SS_TWO_VIEW_COS_1DEG, p.min_triangulated = 50;
    p.max_iterations = 64, p.seed = 99u;
    for (int round = 0; round < 3; round++) {
        std::vector<float> corr((size_t)4 * n), s1((size_t)n, 1.44f);
        for (int k = 0; k < n; k++) {
            observe(s, round == 1, 0.2f, corr.data() + 4 * k);
            if (k % 10 < 3) corr[(size_t)4 * k + 2] = 640.0f * unit(s), corr[(size_t)4 * k + 3] = 480.0f * unit(s);
        }
        if (round == 2) corr[41] = odd[6], corr[402] = odd[7], corr[803] = odd[5];
        std::vector<uint8_t> flag((size_t)n);
        std::vector<ss_map_point> pts((size_t)n);
        ss_two_view_result r;
        ss_tv_problem_host(corr.data(), s1.data(), n, CAM, 2.0736f, p, (uint32_t)round, flag.data(), pts.data(), &r);
        if (r.n_corr != n || r.state < 0 || r.state > 3) return printf("round %d: state %d\n", round, r.state), 1;
        if (round == 0 && (r.model != 1 || r.n_inliers < 150)) return printf("round 0: model %d, %d inliers\n", r.model, r.n_inliers), 1;
        if (round == 1 && r.model != 2) return printf("round 1: model %d\n", r.model), 1;
        int tri = 0;
        for (int k = 0; k < n; k++) tri += flag[(size_t)k] == 3 ? 1 : 0;
        if (tri != r.n_triangulated || (r.state != 0 && tri != 0)) return printf("round %d: %d flags, %d points\n", round, tri, r.n_triangulated), 1;
        steps += (long)p.max_iterations * n;
    }
    /* too few, and a set that does not normalise */
    {
        float few[4 * 7] = {0};
        uint8_t flag[7];
        ss_map_point pts[7];
        float s1[7] = {1, 1, 1, 1, 1, 1, 1};
        ss_two_view_result r;
        ss_tv_problem_host(few, s1, 7, CAM, 2.0f, p, 0u, flag, pts, &r);
        if (r.state != 1) return printf("7 correspondences: state %d\n", r.state), 1;
        std::vector<float> same((size_t)4 * 40, 100.0f), sc((size_t)40, 1.0f);
        std::vector<uint8_t> fl(40);
        std::vector<ss_map_point> pp(40);
        ss_tv_problem_host(same.data(), sc.data(), 40, CAM, 2.0f, p, 0u, fl.data(), pp.data(), &r);
        if (r.state != 2) return printf("one point: state %d\n", r.state), 1;
        steps += 2;
    }
    printf("ok %ld (zero models: %ld H, %ld F; %ld checks)\n", steps, zero_h, zero_f, hyps);
    return 0;
}
