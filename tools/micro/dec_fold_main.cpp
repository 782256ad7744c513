// dec_fold_main.cpp -- a stand-alone host program around the decoder's weight fold (csrc/dec_fold.hip is plain C++), for the host
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/micro/dec_fold_main.cpp cae-lo_amd/csrc/dec_fold.hip -o dec_fold_san
// Every array is a heap block of exactly its size, so a read past the kernel or a write past the folded image is an AddressSanitizer
// report.  The program checks the fold of seeded kernels, for (cin, cout) = (16, 8), (8, 1) and (1, 1), against a second, differently
// written evaluation: UpSampling3D(2) + the 3^3 `same` convolution carried out on an explicit upsampled grid in float64, and the
// folded 2^3 convolution on the source grid, agree on every output voxel of a seeded 4^3 grid, borders included; every class sums
// all 27 taps exactly once; and the argument errors.  Exit status 0 = all checks passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/caelo.h"

static char g_err[512];
void caelo_set_error(const char *fmt, ...) {   // (libcaelo's lives beside the HIP code)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static uint32_t g_seed = 11u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 8388608.0f - 1.0f;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int one(int cin, int cout) {
    const int S = 4, U = 2 * S;
    const size_t cc = (size_t)cin * cout;
    std::unique_ptr<float[]> w(new float[27 * cc]), folded(new float[64 * cc]), x(new float[(size_t)S * S * S * cin]);
    for (size_t i = 0; i < 27 * cc; ++i) w[i] = rnd();
    for (size_t i = 0; i < (size_t)S * S * S * cin; ++i) x[i] = rnd();
    CHECK(caelo_host_decoder_fold(w.get(), cin, cout, folded.get()) == CAELO_OK);
    // every class holds each tap once: the sum over the offsets is the sum over the taps
    for (int p = 0; p < 8; ++p)
        for (size_t e = 0; e < cc; ++e) {
            double a = 0.0, b = 0.0;
            for (int o = 0; o < 8; ++o) a += (double)folded[((size_t)p * 8 + o) * cc + e];
            for (int t = 0; t < 27; ++t) b += (double)w[(size_t)t * cc + e];
            CHECK(fabs(a - b) <= 1e-5);
        }
    double worst = 0.0;
    for (int ux = 0; ux < U; ++ux)
        for (int uy = 0; uy < U; ++uy)
            for (int uz = 0; uz < U; ++uz)
                for (int co = 0; co < cout; ++co) {
                    double direct = 0.0, viafold = 0.0;
                    for (int t = 0; t < 27; ++t) {   // the upsampled grid, zero outside [0, U)
                        const int vx = ux + t / 9 - 1, vy = uy + (t / 3) % 3 - 1, vz = uz + t % 3 - 1;
                        if (vx < 0 || vx >= U || vy < 0 || vy >= U || vz < 0 || vz >= U) continue;
                        for (int ci = 0; ci < cin; ++ci)
                            direct += (double)x[(((size_t)(vx / 2) * S + vy / 2) * S + vz / 2) * cin + ci] * (double)w[((size_t)t * cin + ci) * cout + co];
                    }
                    const int p = (ux & 1) * 4 + (uy & 1) * 2 + (uz & 1);
                    for (int o = 0; o < 8; ++o) {   // the source grid, zero outside [0, S)
                        const int cx = ux / 2 + (o >> 2) + (ux & 1) - 1, cy = uy / 2 + ((o >> 1) & 1) + (uy & 1) - 1, cz = uz / 2 + (o & 1) + (uz & 1) - 1;
                        if (cx < 0 || cx >= S || cy < 0 || cy >= S || cz < 0 || cz >= S) continue;
                        for (int ci = 0; ci < cin; ++ci)
                            viafold += (double)x[(((size_t)cx * S + cy) * S + cz) * cin + ci] * (double)folded[(((size_t)p * 8 + o) * cin + ci) * cout + co];
                    }
                    worst = fmax(worst, fabs(direct - viafold));
                }
    CHECK(worst <= 2e-5);   // the folded weights are rounded to float32 once: <= 2^-24 relative each, a few dozen terms of size <= 1
    return 0;
}

int main() {
    if (one(16, 8) || one(8, 1) || one(1, 1)) return 1;
    std::unique_ptr<float[]> w(new float[27]), f(new float[64]);
    for (int i = 0; i < 27; ++i) w[i] = 1.0f;
    CHECK(caelo_host_decoder_fold(nullptr, 1, 1, f.get()) == CAELO_ERR_ARG && strstr(g_err, "caelo_host_decoder_fold") != nullptr);
    CHECK(caelo_host_decoder_fold(w.get(), 1, 1, nullptr) == CAELO_ERR_ARG);
    CHECK(caelo_host_decoder_fold(w.get(), 0, 1, f.get()) == CAELO_ERR_ARG);
    CHECK(caelo_host_decoder_fold(w.get(), 1, -3, f.get()) == CAELO_ERR_ARG);
    CHECK(caelo_host_decoder_fold(w.get(), 1, 1, f.get()) == CAELO_OK);
    // all-ones kernel: class p, offset o collects (2 - |..|) taps per axis: 1 or 2 each
    for (int p = 0; p < 8; ++p)
        for (int o = 0; o < 8; ++o) {
            int want = 1;
            for (int a = 0; a < 3; ++a) want *= (((p >> a) & 1) == ((o >> a) & 1)) ? 1 : 2;   // p = 0: o = 0 one tap, o = 1 two; p = 1: the reverse
            CHECK(f[p * 8 + o] == (float)want);
        }
    printf("dec_fold ok\n");
    return 0;
}
