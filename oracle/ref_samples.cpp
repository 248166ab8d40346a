// ref_samples.cpp — per-sample records, small films and Poisson solves made by the REFERENCE's own integrators.
//
// Built only in the development container (oracle/Makefile target `ref_samples`): linked against every translation
// unit of the reference's CMakeLists where they lie under /root/reference (render.cpp and parsers/parse_scene.cpp
// included), against rtc_standin.cpp in place of the Embree library and dct_standin.cpp in place of FFTW. Nothing of
// the reference is copied into this repository; grad_path_tracing, path_tracing and fourierSolve are called unmodified
// (they are external functions of the reference's render.cpp and are only declared here).
//
//   ref_samples samples <scene.xml> <count> <stream offset> <out.txt>
//       sample i: pixel (37 i mod W, 91 i mod H), rng = init_pcg32(offset + i); one text line per sample
//       GradPath: x y stream | radiance contrib contribX0 contribX1 contribY0 contribY1 (3 each) prob wX0 wY0 wX1 wY1 | kind margin | state
//       Path:     x y stream | radiance (3) | kind margin | state
//   ref_samples film <scene.xml> <spp> <out.bin>
//       render.cpp's 16x16 tile loop with spp as a parameter (the reference hard-codes 1000 and 256), one
//       init_pcg32(tile) stream per tile, accumulated as render.cpp:311-318 / :107-110. Raw float64: the five buffers
//       img cx0 cy0 cx1 cy1 (GradPath) or img (Path), H*W*3 each, then the per-pixel margin, H*W.
//   ref_samples fourier <w> <h> <alpha> <in.bin> <out.bin>
//       in: c, gx, gy (raw float64, H*W*3 each); out: fourierSolve's result.
//
// Allocation: the reference's make_mipmap (src/mipmap.h:33-43) halves a one-texel-high level of a wider image to
// max(0, 1) = 1 rows and reads row 1 of it, one whole level past the end of its buffer. So that this read lands in
// memory of ours, operator new here hands out twice the bytes asked for (+64) and fills the second half with the double
// in the environment variable GDPT_REF_PAD (default 0). gen_golden.py runs everything twice, with two values, and marks
// what differs as `undefined`: there the reference's answer is no function of its source.
//
// margin: the minimum, over the rays of a sample, of what rtc_standin.cpp recorded (how close a ray's answer was to
// changing). All driver code here is this repository's own.
// pcg.h defines the two full specialisations of next_pcg32_real without `inline`, so a second translation unit that includes it
// would define them again beside render.cpp's. Here the template and its specialisations get a name of this unit's own; the types
// and init_pcg32 are the reference's.
#define next_pcg32_real next_pcg32_real_in_ref_samples
#include "pcg.h"
#undef next_pcg32_real
#include "camera.h"
#include "intersection.h"
#include "parsers/parse_scene.h"
#include "scene.h"
#include "spectrum.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <string>
#include <vector>

// defined in the reference's render.cpp (path_tracing.h is included there and nowhere else)
Spectrum path_tracing(const Scene &scene, int x, int y, pcg32_state &rng);
GraidentPTRadiance grad_path_tracing(const Scene &scene, int x, int y, pcg32_state &rng);
void fourierSolve(int width, int height, const double *imgData, const double *imgGradX, const double *imgGradY, double dataCost, double *imgOut);

extern "C" void rtc_standin_margin_reset(void);
extern "C" double rtc_standin_margin(void);
extern "C" int rtc_standin_margin_kind(void);
extern "C" int rtc_standin_first_ray(float org_dir[6]);

// path_tracing draws its two sub-pixel numbers inside one constructor call (path_tracing.h:21-22), so their order is the
// compiler's choice. The fixtures are defined with x first (clang, which the reference was developed with; oracle/Makefile
// compiles render.cpp accordingly): one Path sample, its first ray against sample_primary with the first draw given to x.
static void require_x_first(const Scene &scene) {
    if (scene.options.integrator != Integrator::Path) return;
    const int w = scene.camera.width, h = scene.camera.height, x = w / 3, y = h / 3;
    pcg32_state rng = init_pcg32(0), probe = rng;
    double r0 = next_pcg32_real_in_ref_samples<Real>(probe), r1 = next_pcg32_real_in_ref_samples<Real>(probe);
    Ray want = sample_primary(scene.camera, Vector2((x + r0) / w, (y + r1) / h));
    rtc_standin_margin_reset();
    path_tracing(scene, x, y, rng);
    float got[6];
    if (!rtc_standin_first_ray(got) || got[3] != (float)want.dir.x || got[4] != (float)want.dir.y || got[5] != (float)want.dir.z) {
        fprintf(stderr, "ref_samples: path_tracing does not draw x first: compile the reference's render.cpp with clang (oracle/Makefile, ORDER_CXX)\n");
        exit(4);
    }
}

static double pad_value() {
    static const double v = [] { const char *e = getenv("GDPT_REF_PAD"); return e ? atof(e) : 0.0; }();
    return v;
}
void *operator new(size_t n) {
    size_t body = (n + 7) & ~(size_t)7, total = 2 * body + 64;
    char *p = (char *)malloc(total);
    if (!p) throw std::bad_alloc();
    const double v = pad_value();
    for (size_t off = body; off + sizeof(double) <= total; off += sizeof(double)) memcpy(p + off, &v, sizeof(double));
    return p;
}
void *operator new[](size_t n) { return operator new(n); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

static void put3(FILE *f, const Spectrum &s) { fprintf(f, " %.17g %.17g %.17g", s.x, s.y, s.z); }

static int run_samples(const Scene &scene, int count, unsigned long long offset, const char *out_path) {
    FILE *f = fopen(out_path, "w");
    if (!f) return 2;
    const int w = scene.camera.width, h = scene.camera.height;
    const bool grad = scene.options.integrator == Integrator::GradPath;
    for (int i = 0; i < count; i++) {
        int x = (int)((37LL * i) % w), y = (int)((91LL * i) % h);
        pcg32_state rng = init_pcg32(offset + (unsigned long long)i);
        rtc_standin_margin_reset();
        fprintf(f, "%d %d %llu", x, y, offset + (unsigned long long)i);
        if (grad) {
            GraidentPTRadiance r = grad_path_tracing(scene, x, y, rng);
            put3(f, r.radiance); put3(f, r.contrib); put3(f, r.contribX0); put3(f, r.contribX1); put3(f, r.contribY0); put3(f, r.contribY1);
            fprintf(f, " %.17g %.17g %.17g %.17g %.17g", r.prob, r.wX0, r.wY0, r.wX1, r.wY1);
        } else {
            put3(f, path_tracing(scene, x, y, rng));
        }
        fprintf(f, " %d %.17g %llu\n", rtc_standin_margin_kind(), rtc_standin_margin(), (unsigned long long)rng.state);
    }
    fclose(f);
    return 0;
}

static int run_film(const Scene &scene, int spp, const char *out_path) {
    const int w = scene.camera.width, h = scene.camera.height;
    const bool grad = scene.options.integrator == Integrator::GradPath;
    std::vector<Spectrum> img((size_t)w * h, make_zero_spectrum()), cx0(img), cy0(img), cx1(img), cy1(img);
    std::vector<double> margin((size_t)w * h, 0.0);
    const int tile_size = 16;
    const int ntx = (w + tile_size - 1) / tile_size, nty = (h + tile_size - 1) / tile_size;
    for (int ty = 0; ty < nty; ty++) for (int tx = 0; tx < ntx; tx++) {
        pcg32_state rng = init_pcg32(ty * ntx + tx);
        int x0 = tx * tile_size, x1 = std::min(x0 + tile_size, w), y0 = ty * tile_size, y1 = std::min(y0 + tile_size, h);
        for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) {
            size_t p = (size_t)y * w + x;
            rtc_standin_margin_reset();
            if (grad) {
                Spectrum r = make_zero_spectrum(), rdX0 = r, rdX1 = r, rdY0 = r, rdY1 = r;
                for (int s = 0; s < spp; s++) {
                    GraidentPTRadiance g = grad_path_tracing(scene, x, y, rng);
                    if (g.prob > 0.0) {
                        r = r + g.radiance / Real(spp);
                        rdX0 = rdX0 + (g.contrib - g.contribX0) * (g.wX0 / (g.prob * Real(spp)));
                        rdY0 = rdY0 + (g.contrib - g.contribY0) * (g.wY0 / (g.prob * Real(spp)));
                        rdX1 = rdX1 + (g.contribX1 - g.contrib) * (g.wX1 / (g.prob * Real(spp)));
                        rdY1 = rdY1 + (g.contribY1 - g.contrib) * (g.wY1 / (g.prob * Real(spp)));
                    }
                }
                img[p] += r; cx0[p] += rdX0; cy0[p] += rdY0; cx1[p] += rdX1; cy1[p] += rdY1;
            } else {
                Spectrum radiance = make_zero_spectrum();
                for (int s = 0; s < spp; s++) radiance += path_tracing(scene, x, y, rng);
                img[p] = radiance / Real(spp);
            }
            margin[p] = rtc_standin_margin();
        }
    }
    FILE *f = fopen(out_path, "wb");
    if (!f) return 2;
    static_assert(sizeof(Spectrum) == 3 * sizeof(double), "Spectrum is three doubles");
    fwrite(img.data(), sizeof(Spectrum), img.size(), f);
    if (grad) for (auto *b : {&cx0, &cy0, &cx1, &cy1}) fwrite(b->data(), sizeof(Spectrum), b->size(), f);
    fwrite(margin.data(), sizeof(double), margin.size(), f);
    fclose(f);
    return 0;
}

static int run_fourier(int w, int h, double alpha, const char *in_path, const char *out_path) {
    size_t n = (size_t)w * h * 3;
    std::vector<double> in(3 * n), out(n, 0.0);
    FILE *f = fopen(in_path, "rb");
    if (!f || fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
    fclose(f);
    fourierSolve(w, h, in.data(), in.data() + n, in.data() + 2 * n, alpha, out.data());
    f = fopen(out_path, "wb");
    if (!f) return 2;
    fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "fourier" && argc == 7) return run_fourier(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), argv[5], argv[6]);
    if ((mode == "samples" && argc == 6) || (mode == "film" && argc == 5)) {
        RTCDevice device = rtcNewDevice(nullptr);
        std::unique_ptr<Scene> scene = parse_scene(argv[2], device);
        if (scene->options.integrator != Integrator::GradPath && scene->options.integrator != Integrator::Path) return 3;
        require_x_first(*scene);
        int rc = mode == "samples" ? run_samples(*scene, atoi(argv[3]), strtoull(argv[4], nullptr, 10), argv[5])
                                   : run_film(*scene, atoi(argv[3]), argv[4]);
        scene.reset();
        rtcReleaseDevice(device);
        return rc;
    }
    fprintf(stderr, "usage: ref_samples samples <xml> <count> <offset> <out> | film <xml> <spp> <out> | fourier <w> <h> <alpha> <in> <out>\n");
    return 1;
}
