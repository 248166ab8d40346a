// dct_standin.cpp — the five fftw_* entry points that the reference's fourierSolve calls, by definition.
//
// Built only where the reference tree is present (oracle/Makefile target `ref_samples`), against the fftw3.h that lies
// in that tree; the library itself cannot be configured there. Everything in this file is this repository's own code.
//
// fftw_plan_r2r_2d accepts REDFT00 in both dimensions and nothing else. fftw_execute is the direct O(n^2)-per-line
// DCT-I in long double, unnormalised as FFTW's is:  Y[k] = X[0] + (-1)^k X[n-1] + 2 sum_{j=1}^{n-2} X[j] cos(pi j k / (n-1)).
// This pins what the reference wraps around the transform (right-hand side, eigenvalue, DC override, scaling); the
// transform itself stays pinned by this definition and by scipy's dctn(type=1).
#include <fftw3.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct fftw_plan_s {
    int n0, n1;             // rows, columns (row-major)
    double *in, *out;
};

namespace {

void dct1_line(const std::vector<long double> &cos_tab, int n, const long double *x, int stride, long double *y) {
    // cos_tab[m] = cos(pi m / (n-1)) for m in [0, 2(n-1)); the argument j k is reduced modulo 2(n-1) exactly
    const int period = 2 * (n - 1);
    for (int k = 0; k < n; k++) {
        long double acc = x[0] + ((k & 1) ? -x[(size_t)(n - 1) * stride] : x[(size_t)(n - 1) * stride]);
        for (int j = 1; j < n - 1; j++) acc += 2.0L * x[(size_t)j * stride] * cos_tab[(size_t)(((long long)j * k) % period)];
        y[k] = acc;
    }
}

std::vector<long double> make_cos_tab(int n) {
    const int period = 2 * (n - 1);
    std::vector<long double> t((size_t)period);
    for (int m = 0; m < period; m++) t[(size_t)m] = cosl(3.14159265358979323846264338327950288L * m / (n - 1));
    return t;
}

} // namespace

extern "C" {

void *fftw_malloc(size_t n) { return malloc(n); }
void fftw_free(void *p) { free(p); }

fftw_plan fftw_plan_r2r_2d(int n0, int n1, double *in, double *out, fftw_r2r_kind kind0, fftw_r2r_kind kind1, unsigned) {
    if (kind0 != FFTW_REDFT00 || kind1 != FFTW_REDFT00 || n0 < 2 || n1 < 2) {
        fprintf(stderr, "dct_standin: only REDFT00 x REDFT00 with both sizes >= 2 is provided\n");
        abort();
    }
    fftw_plan p = new fftw_plan_s;
    p->n0 = n0; p->n1 = n1; p->in = in; p->out = out;
    return p;
}

void fftw_execute(const fftw_plan p) {
    const int h = p->n0, w = p->n1;
    std::vector<long double> a((size_t)w * h), b((size_t)w * h), line((size_t)(w > h ? w : h));
    for (size_t i = 0; i < a.size(); i++) a[i] = p->in[i];
    const std::vector<long double> cw = make_cos_tab(w), ch = make_cos_tab(h);
    for (int y = 0; y < h; y++) dct1_line(cw, w, &a[(size_t)y * w], 1, &b[(size_t)y * w]);
    for (int x = 0; x < w; x++) {
        dct1_line(ch, h, &b[(size_t)x], w, line.data());
        for (int y = 0; y < h; y++) a[(size_t)y * w + x] = line[(size_t)y];
    }
    for (size_t i = 0; i < a.size(); i++) p->out[i] = (double)a[i];
}

void fftw_destroy_plan(fftw_plan p) { delete p; }

} // extern "C"
