// correct.hip -- the vertical-angle calibration of a scan (Transformations.py:28-39 CorrectPC; BatchPreprocess.py:70-88), device resident.
//
// Reference behaviour restated here (never its code): every point p is rotated by CalibAngle about the axis p x z^.  Per point the
// reference forms, in float32 (NumPy >= 2 arithmetic, NEP 50: the Python scalars are weak), every operation rounded on its own:
//   r = cross(p, (0,0,1)) = (y*1 - z*0, z*0 - x*1, x*0 - y*0)              Transformations.py:31
//   n = sqrt((r0^2 + r1^2) + r2^2),  v = r / n                              :32,:35
//   q = (c, v0*s, v1*s, v2*s),  s = float32(sin(a/2)), c = float32(cos(a/2))   AngleAxis2Quatern :264-272
//   R from q, left to right: R00 = (1 - (2*q2)*q2) - (2*q3)*q3, ...         Quatern2RotMat :241-252
//   p' = dot(R, p)                                                          :38
// Steps up to R are the reference's bits.  dot(R, p) is a 3 x 3 sgemv of the host's BLAS, whose summation order is its own: here
// p'_i = (R_i0*x + R_i1*y) + R_i2*z, no contraction (DESIGN.md 5.8 gives the bound between the two).  A point on the z axis has
// n = 0: v, R and p' are NaN and stay NaN, as in the Python reference; the frame then reports CAELO_ST_NONFINITE downstream.
//
// One thread per point, blockIdx.y = frame.  The kernel moves 32 B per point and computes ~60 flops: memory bound.  With stride 4 a
// lane loads and stores one 16-byte point (a wave covers 1 KiB of consecutive addresses per instruction); with stride 3 (or a
// buffer that is not 16-byte aligned) three dword loads per lane, consecutive lanes 12 B apart.
#include <math.h>

#include "caelo_internal.h"

#pragma clang fp contract(off)

struct CorrectSet {   // blockIdx.y = frame
    const float *in[CAELO_FB_MAX];
    float *out[CAELO_FB_MAX];
    long long n[CAELO_FB_MAX];
    float s, c;       // float32(sin(a / 2)), float32(cos(a / 2)), computed on the host in double
};

// `/` and sqrtf are IEEE correctly rounded here (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; no fast-math flag in the
// Makefile), f32 denormals are kept.
__device__ inline void correct_point(const float x, const float y, const float z, const float s, const float c, float &ox, float &oy,
                                     float &oz) {
    const float r0 = y * 1.0f - z * 0.0f, r1 = z * 0.0f - x * 1.0f, r2 = x * 0.0f - y * 0.0f;
    const float n = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
    const float v0 = r0 / n, v1 = r1 / n, v2 = r2 / n;
    const float q0 = c, q1 = v0 * s, q2 = v1 * s, q3 = v2 * s;
    const float R00 = (1.0f - (2.0f * q2) * q2) - (2.0f * q3) * q3;
    const float R01 = (2.0f * q1) * q2 - (2.0f * q3) * q0;
    const float R02 = (2.0f * q2) * q0 + (2.0f * q3) * q1;
    const float R10 = (2.0f * q1) * q2 + (2.0f * q3) * q0;
    const float R11 = (1.0f - (2.0f * q1) * q1) - (2.0f * q3) * q3;
    const float R12 = (2.0f * q2) * q3 - (2.0f * q1) * q0;
    const float R20 = (2.0f * q1) * q3 - (2.0f * q2) * q0;
    const float R21 = (2.0f * q2) * q3 + (2.0f * q1) * q0;
    const float R22 = (1.0f - (2.0f * q1) * q1) - (2.0f * q2) * q2;
    ox = (R00 * x + R01 * y) + R02 * z;
    oy = (R10 * x + R11 * y) + R12 * z;
    oz = (R20 * x + R21 * y) + R22 * z;
}

// VEC: stride 4, both buffers 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(256) k_correct_pc(const CorrectSet a, const int stride) {
    const int f = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n[f]) return;
    if (VEC) {
        const float4 p = reinterpret_cast<const float4 *>(a.in[f])[i];
        float4 o;
        correct_point(p.x, p.y, p.z, a.s, a.c, o.x, o.y, o.z);
        o.w = p.w;   // intensity: the same bits
        reinterpret_cast<float4 *>(a.out[f])[i] = o;
    } else {
        const float *p = a.in[f] + (size_t)i * stride;
        float *o = a.out[f] + (size_t)i * stride;
        float ox, oy, oz;
        correct_point(p[0], p[1], p[2], a.s, a.c, ox, oy, oz);
        o[0] = ox; o[1] = oy; o[2] = oz;
        if (stride == 4) reinterpret_cast<uint32_t *>(o)[3] = reinterpret_cast<const uint32_t *>(p)[3];
    }
}

static void correct_angle(double deg, float *s, float *c) {
    const double a = deg * 3.141592653589793 / 180.0;   // CalibAngle * math.pi / 180, left to right
    const double h = a / 2;
    *s = (float)sin(h);
    *c = (float)cos(h);
}

static int correct_launch(CorrectSet &a, int n_frames, int stride, double deg, hipStream_t s) {
    long long most = 0;
    bool vec = stride == 4;
    for (int f = 0; f < n_frames; ++f) {
        most = a.n[f] > most ? a.n[f] : most;
        vec = vec && (((uintptr_t)a.in[f] | (uintptr_t)a.out[f]) & 15u) == 0;
    }
    if (most == 0) return CAELO_OK;
    correct_angle(deg, &a.s, &a.c);
    const dim3 grid((unsigned)((most + 255) / 256), (unsigned)n_frames);
    if (vec) k_correct_pc<true><<<grid, 256, 0, s>>>(a, stride);
    else k_correct_pc<false><<<grid, 256, 0, s>>>(a, stride);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_set_calib_angle(caelo_ctx *c, double deg) {
    CAELO_REQUIRE(c, "null argument");
    CAELO_REQUIRE(isfinite(deg), "the calibration angle must be finite");
    c->calib_angle = deg;
    return CAELO_OK;
}

CAELO_API double caelo_get_calib_angle(caelo_ctx *c) { return c ? c->calib_angle : 0.0; }

CAELO_API int caelo_correct_pc(caelo_ctx *c, const float *pc, int64_t n, int stride, double calib_angle_deg, float *out, void *stream) {
    CAELO_REQUIRE(c, "null argument");
    CAELO_REQUIRE(stride == 3 || stride == 4, "stride must be 3 or 4");
    CAELO_REQUIRE(n >= 0 && n < (1LL << 31), "bad point count");
    CAELO_REQUIRE(isfinite(calib_angle_deg), "the calibration angle must be finite");
    if (n == 0) return CAELO_OK;
    CAELO_REQUIRE(pc && out, "null argument");
    const uintptr_t bytes = (uintptr_t)n * stride * 4, a = (uintptr_t)pc, b = (uintptr_t)out;
    CAELO_REQUIRE(a + bytes <= b || b + bytes <= a, "out may not alias pc");
    CorrectSet set = {};
    set.in[0] = pc; set.out[0] = out; set.n[0] = n;
    return correct_launch(set, 1, stride, calib_angle_deg, caelo_stream(stream));
}

// ---- CAELO_EXTRACT_CORRECT_PC: the scans of a frame set corrected into their maps' storage, one launch, before anything reads them
int correct_prepare(caelo_voxmap *const *maps, int n) {
    for (int i = 0; i < n; ++i) {
        caelo_voxmap *m = maps[i];
        if (m->corr) continue;
        if (hipMalloc((void **)&m->corr, (size_t)m->max_points * 16) != hipSuccess) {
            m->corr = nullptr;
            caelo_set_error("correct_prepare: no device memory for a corrected scan (%lld points)", (long long)m->max_points);
            return CAELO_ERR_HIP;
        }
    }
    return CAELO_OK;
}

int correct_set(const caelo_extract_args *args, int n, hipStream_t s) {
    CorrectSet set = {};
    for (int i = 0; i < n; ++i) {
        CAELO_REQUIRE(args[i].map->corr && args[i].n <= args[i].map->max_points, "internal: correct_prepare was not called for this set");
        set.in[i] = args[i].pc; set.out[i] = args[i].map->corr; set.n[i] = args[i].n;
    }
    return correct_launch(set, n, 4, args[0].ctx->calib_angle, s);
}
