// loopclose_main.cpp -- a stand-alone host program around the loop-closure host twins (csrc/loopclose_host.hip is plain C++), for the
// host sanitizers:
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/micro/loopclose_main.cpp cae-lo_amd/csrc/loopclose_host.hip -o loopclose_san
// Every array is a heap block of exactly its size, so a read or write past one is an AddressSanitizer report.  The program runs the
// capacity cases (every point of a full cloud counted, points on the outermost ring and the last sector, every one of the 8 result slots
// and the dense images filled, the largest shift) and the empty ones (no frame, no point, an all-empty image as query and as candidate,
// an empty query range, no candidate at all) and the argument errors.  Exit status 0 = all checks passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../../include/caelo.h"

static char g_err[512];
void caelo_set_error(const char *fmt, ...) {   // (libcaelo's lives beside the HIP code)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static uint32_t g_seed = 5u;
static float rnd() {   // [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 16777216.0f;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    // ---- descriptors: F frames of exactly ld points with C columns; frame 1 is empty, frame 2 a rolled copy of frame 0
    const int F = 12, ld = 257;
    for (int C = 3; C <= 4; ++C) {
        std::unique_ptr<float[]> pts(new float[(size_t)F * ld * C]);
        std::unique_ptr<int32_t[]> n_pts(new int32_t[F]);
        std::unique_ptr<float[]> sc(new float[(size_t)F * 1200]), u(new float[(size_t)F * 1200]);
        std::unique_ptr<uint64_t[]> valid(new uint64_t[F]);
        for (int f = 0; f < F; ++f) {
            n_pts[f] = f == 1 ? 0 : (f == 3 ? ld + 9 : ld);   // more than ld counts as ld
            for (int p = 0; p < ld; ++p) {
                const double r = p == 0 ? 79.999 : 1.0 + 78.0 * rnd(), th = p == 1 ? 6.28318 : 6.2831 * rnd();
                float *q = &pts[((size_t)f * ld + p) * C];
                q[0] = (float)(r * cos(th)); q[1] = (float)(r * sin(th)); q[2] = 4.0f * rnd() - 3.0f;
                if (C == 4) q[3] = rnd();
                if (p == 2) q[0] = NAN;
                if (p == 3) q[2] = INFINITY;
                if (p == 4) { q[0] = 0.0f; q[1] = 0.0f; }
                if (p == 5) { q[0] = 80.0f; q[1] = 0.0f; }
            }
        }
        CHECK(caelo_host_scan_context(pts.get(), ld, C, n_pts.get(), F, sc.get(), u.get(), valid.get()) == CAELO_OK);
        CHECK(valid[1] == 0 && valid[0] != 0 && (valid[0] >> 60) == 0);
        for (int k = 0; k < 1200; ++k) CHECK(sc[1200 + k] == 0.0f && u[1200 + k] == 0.0f);
        CHECK(caelo_host_scan_context(pts.get(), ld, C, n_pts.get(), 0, sc.get(), u.get(), valid.get()) == CAELO_OK);   // no frame
        CHECK(caelo_host_scan_context(pts.get(), ld, 5, n_pts.get(), F, sc.get(), u.get(), valid.get()) == CAELO_ERR_ARG);
        CHECK(caelo_host_scan_context(nullptr, ld, C, n_pts.get(), F, sc.get(), u.get(), valid.get()) == CAELO_ERR_ARG);
        // frame 11 := frame 0 seen 59 sectors on: u_11[c] = u_0[c + 59]
        for (int c = 0; c < 60; ++c) memcpy(&u[11 * 1200 + c * 20], &u[((c + 59) % 60) * 20], 80);
        valid[11] = 0;
        for (int c = 0; c < 60; ++c) valid[11] |= ((valid[0] >> ((c + 59) % 60)) & 1ull) << c;
        // ---- search: every slot filled (query 11 has 11 candidates at min_gap 1, k = 8), dense images, the empty frame 1
        const int k = 8;
        std::unique_ptr<int32_t[]> cand(new int32_t[(size_t)F * k]), shift(new int32_t[(size_t)F * k]);
        std::unique_ptr<float[]> dist(new float[(size_t)F * k]), dd(new float[(size_t)F * F]);
        std::unique_ptr<int8_t[]> ds(new int8_t[(size_t)F * F]);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F, 1, k, INFINITY, 1, cand.get(), dist.get(), shift.get(), dd.get(), ds.get()) == CAELO_OK);
        CHECK(cand[11 * k] == 0 && shift[11 * k] == 59 && fabsf(dist[11 * k]) < 1e-5f);
        CHECK(cand[11 * k + 7] >= 0 && cand[0] == -1 && shift[0] == -1 && isinf(dist[0]));
        CHECK(ds[11 * F + 1] == -1 && isinf(dd[11 * F + 1]));                 // the empty frame as candidate
        for (int t = 0; t < k; ++t) CHECK(cand[1 * k + t] == -1);             // ... and as query
        for (int t = 1; t < k; ++t) CHECK(dist[11 * k + t] >= dist[11 * k + t - 1]);
        // an empty query range, a range of one, no candidate at all (min_gap = F), min_cols = 60
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 5, 5, 1, k, INFINITY, 1, cand.get(), dist.get(), shift.get(), nullptr, nullptr) == CAELO_OK);
        std::unique_ptr<int32_t[]> c1(new int32_t[1]), s1(new int32_t[1]);
        std::unique_ptr<float[]> d1(new float[1]), dd1(new float[F]);
        std::unique_ptr<int8_t[]> ds1(new int8_t[F]);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 11, 12, 1, 1, 0.5f, 1, c1.get(), d1.get(), s1.get(), dd1.get(), ds1.get()) == CAELO_OK);
        CHECK(c1[0] == 0 && s1[0] == 59 && ds1[0] == 59 && ds1[11] == -1);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 11, 12, F, 1, INFINITY, 1, c1.get(), d1.get(), s1.get(), nullptr, nullptr) == CAELO_OK);
        CHECK(c1[0] == -1);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 11, 12, 1, 1, INFINITY, 60, c1.get(), d1.get(), s1.get(), nullptr, nullptr) == CAELO_OK);
        // the argument errors
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F, 1, 9, INFINITY, 1, cand.get(), dist.get(), shift.get(), nullptr, nullptr) == CAELO_ERR_ARG);
        CHECK(strstr(g_err, "caelo_host_loop_search") != nullptr);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F, 0, 1, INFINITY, 1, cand.get(), dist.get(), shift.get(), nullptr, nullptr) == CAELO_ERR_ARG);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F, 1, 1, INFINITY, 61, cand.get(), dist.get(), shift.get(), nullptr, nullptr) == CAELO_ERR_ARG);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F + 1, 1, 1, INFINITY, 1, cand.get(), dist.get(), shift.get(), nullptr, nullptr) == CAELO_ERR_ARG);
        CHECK(caelo_host_loop_search(u.get(), valid.get(), F, 0, F, 1, 1, INFINITY, 1, cand.get(), dist.get(), shift.get(), dd.get(), nullptr) == CAELO_ERR_ARG);
    }
    printf("loopclose ok\n");
    return 0;
}
