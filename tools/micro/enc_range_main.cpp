// enc_range_main.cpp -- a stand-alone host program around the encoder's range guard (csrc/enc_range.hip is plain C++), for the host
// sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/micro/enc_range_main.cpp cae-lo_amd/csrc/enc_range.hip -o enc_range_san
// Every array is a heap block of exactly its size, so a read past a layer's weights is an AddressSanitizer report.  The program checks
// the bounds against a second, differently written evaluation, the refusal of an over-range relu model (layer named, bounds still
// filled in), that a tanh hidden stack is never refused, and the argument errors.  Exit status 0 = all checks passed.
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

static const size_t N_IN[5] = {27, 27 * 8, 27 * 16, 2048, 200}, N_OUT[5] = {8, 16, 32, 200, 20};

struct Model {
    std::unique_ptr<float[]> a[10];
    const float *p(int i) const { return a[i].get(); }
};

static Model make(uint32_t seed, float scale2) {
    Model m;
    for (int l = 0; l < 5; ++l) {
        m.a[2 * l].reset(new float[N_IN[l] * N_OUT[l]]);
        m.a[2 * l + 1].reset(new float[N_OUT[l]]);
        const float lim = sqrtf(6.0f / (float)(N_IN[l] + (l < 3 ? 27 : 1) * N_OUT[l])) * (l == 1 ? scale2 : 1.0f);
        for (size_t i = 0; i < N_IN[l] * N_OUT[l]; ++i) {
            seed = seed * 1664525u + 1013904223u;
            m.a[2 * l][i] = lim * ((float)(seed >> 8) / 8388608.0f - 1.0f);
        }
        for (size_t i = 0; i < N_OUT[l]; ++i) {
            seed = seed * 1664525u + 1013904223u;
            m.a[2 * l + 1][i] = 0.5f * ((float)(seed >> 8) / 8388608.0f - 1.0f);
        }
    }
    return m;
}

static int range(const Model &m, int h, int c, double *out) {
    return caelo_host_encoder_range(m.p(0), m.p(1), m.p(2), m.p(3), m.p(4), m.p(5), m.p(6), m.p(7), m.p(8), m.p(9), h, c, out);
}

static void expect(const Model &m, int h, int c, double *want) {   // the per-channel recurrence, row by row into column sums
    std::vector<double> prev(1, 1.0);
    for (int l = 0; l < 5; ++l) {
        std::vector<double> col(N_OUT[l], 0.0);
        for (size_t k = 0; k < N_IN[l]; ++k)
            for (size_t o = 0; o < N_OUT[l]; ++o) col[o] += fabs((double)m.p(2 * l)[k * N_OUT[l] + o]) * prev[k % prev.size()];
        double worst = 0.0;
        for (size_t o = 0; o < N_OUT[l]; ++o) {
            col[o] = (l < 4 ? h : c) == CAELO_ACT_TANH ? 1.0 : col[o] + fabs((double)m.p(2 * l + 1)[o]);
            worst = fmax(worst, col[o]);
        }
        want[l] = worst;
        prev = col;
    }
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    const int hs[2] = {CAELO_ACT_TANH, CAELO_ACT_RELU}, cs[2] = {CAELO_ACT_TANH, CAELO_ACT_LINEAR};
    const Model sane = make(7u, 1.0f), wild = make(7u, 1.0e4f);
    for (int h : hs)
        for (int c : cs) {
            double got[5], want[5];
            CHECK(range(sane, h, c, got) == 0);
            expect(sane, h, c, want);
            for (int l = 0; l < 5; ++l) CHECK(fabs(got[l] - want[l]) <= 1e-12 * want[l]);
            const int rc = range(wild, h, c, got);
            expect(wild, h, c, want);
            for (int l = 0; l < 5; ++l) CHECK(fabs(got[l] - want[l]) <= 1e-12 * want[l]);
            if (h == CAELO_ACT_TANH) CHECK(rc == 0);   // a tanh hidden stack is never refused
            else CHECK(rc == 2 && want[1] > 65504.0 && strstr(g_err, "conv3d_2") != nullptr);
        }
    double out[5];
    CHECK(range(sane, 3, CAELO_ACT_TANH, out) == CAELO_ERR_ARG);
    CHECK(range(sane, CAELO_ACT_LINEAR, CAELO_ACT_TANH, out) == CAELO_ERR_ARG);
    CHECK(range(sane, CAELO_ACT_RELU, CAELO_ACT_RELU, out) == CAELO_ERR_ARG);
    CHECK(range(sane, CAELO_ACT_RELU, CAELO_ACT_LINEAR, nullptr) == CAELO_ERR_ARG);
    CHECK(caelo_host_encoder_range(nullptr, sane.p(1), sane.p(2), sane.p(3), sane.p(4), sane.p(5), sane.p(6), sane.p(7), sane.p(8),
                                   sane.p(9), 0, 0, out) == CAELO_ERR_ARG);
    printf("enc_range ok\n");
    return 0;
}
