/*
 * ss_bow_merge.h -- L1Scoring::score of one query vector against one stored vector (the rule: include/sendslam_orb.h,
 * ss_bow_score_device): the wave form k_bow_score (ss_bow.hip) and k_place_score (ss_place.hip) run, and the sequential form the
 * host twin of the place recognition and its sanitizer program run.  Both look every stored word up in the query by the same
 * binary search and add the terms of the common words in ascending stored position, one double addition at a time, so they agree
 * bit for bit on any input, ascending or not.  Compile with -ffp-contract=off.
 */
#ifndef SS_BOW_MERGE_H
#define SS_BOW_MERGE_H

#include <math.h>
#include <stdint.h>

#include "ss_float_steps.h" /* SS_HD */

/* the place of word wd in the ascending q_word[0 .. nq), or -1 */
SS_HD int ss_bow_find(const int32_t *q_word, int nq, int32_t wd)
{
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q_word[mid] < wd) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nq && q_word[lo] == wd) ? lo : -1;
}

/* one common word's term: three double operations left to right */
SS_HD double ss_bow_term(double x, double y) { return fabs(x - y) - fabs(x) - fabs(y); }

/* what the score is once the terms are summed; nq, nd: the clamped counts */
SS_HD double ss_bow_close(double s, int nq, int nd) { return (nq == 0 || nd == 0) ? 0.0 : -s / 2.0; }

/* the sequential form */
SS_HD double ss_bow_score_seq(const int32_t *q_word, const double *q_value, int nq, const int32_t *d_word, const double *d_value, int nd)
{
    double s = 0.0;
    for (int j = 0; j < nd && nq > 0; j++) {
        const int at = ss_bow_find(q_word, nq, d_word[j]);
        if (at >= 0) s += ss_bow_term(q_value[at], d_value[j]);
    }
    return ss_bow_close(s, nq, nd);
}

#if defined(__HIPCC__)
/* the wave form: all 64 lanes of a wave call it with the same arguments; every lane returns the score */
__device__ __forceinline__ double ss_bow_score_wave(const int32_t *q_word, const double *q_value, int nq, const int32_t *dw, const double *dv, int nd, int lane)
{
    double s = 0.0;
    for (int base = 0; base < nd && nq > 0; base += 64) {
        const int j = base + lane;
        bool common = false;
        double term = 0.0;
        if (j < nd) {
            const int at = ss_bow_find(q_word, nq, dw[j]);
            if (at >= 0) {
                term = ss_bow_term(q_value[at], dv[j]);
                common = true;
            }
        }
        unsigned long long mask = __ballot(common);
        while (mask) { /* ascending lanes = ascending words */
            const int l = __ffsll((long long)mask) - 1;
            s += __shfl(term, l);
            mask &= mask - 1;
        }
    }
    return ss_bow_close(s, nq, nd);
}
#endif

#endif
