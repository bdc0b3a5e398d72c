/* sst_two_view (csrc/ss_track.cpp, the bounded tracker's own two-view reconstruction) on correspondences read from a file: int32 n,
 * then n x 4 float32 (u1 v1 u2 v2).  Prints the number of triangulated points, the model (1 F, 2 H), R (9) and t (3).
 * usage: two_view_vs_track corr.bin fx fy cx cy */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_track.h"

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0) return 3;
    std::vector<float> c((size_t)4 * n);
    if (fread(c.data(), 4, c.size(), f) != c.size()) return 3;
    fclose(f);
    const sst_camera cam = {atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), 0.0, 0.0, 0.0, 0.0};
    std::vector<double> x1((size_t)2 * n), x2((size_t)2 * n), p3;
    for (int i = 0; i < n; i++) x1[2 * i] = c[4 * i], x1[2 * i + 1] = c[4 * i + 1], x2[2 * i] = c[4 * i + 2], x2[2 * i + 1] = c[4 * i + 3];
    std::vector<uint8_t> tri;
    double R[9] = {0}, t[3] = {0};
    int model = 0;
    const int got = sst_two_view(cam, n, x1.data(), x2.data(), R, t, tri, p3, &model);
    printf("%d %d", got, model);
    for (double v : R) printf(" %.17g", v);
    for (double v : t) printf(" %.17g", v);
    printf("\n");
    return 0;
}
