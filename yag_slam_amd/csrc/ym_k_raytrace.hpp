// ym_k_raytrace.hpp -- virtual scans from an occupancy image: the pixel walk of the reference's trace_ray
// (/root/reference/yag_slam/raytracing.py:63-88), every (viewpoint, angle) pair of one call in one launch.
//
// The walk, in pixel units (x = column, y = row), as numba runs it: the point is a jitclass with float32 fields
// (raytracing.py:21), so every assignment rounds to float32 while the arithmetic runs in float64.
//   x, y = f32(sx), f32(sy)
//   loop: val = img[rint(y), rint(x)]                              np.round: half to even on the float32 value
//         x, y = f32(f64(x) + c), f32(f64(y) + s)                   the point advances once more after a hit
//         if val < 210 and val > 180: x, y = f32(f64(x) + 1000 c), f32(f64(y) + 1000 s)     "unknown": jump
//         stop if val < 210, or rint(y) < 1 or rint(x) < 1 or rint(x) >= w - 1 or rint(y) >= h - 1
// (c, s) come from the caller's table (no trig on the device), the library is built with -ffp-contract=off (a fused
// x + 1000 c would round differently).  The first read is at the start pixel, before any bounds test: the host
// rejects starts whose rounded pixel lies outside the image.
//
// Termination: the host admits images of at most 65536 x 65536 pixels and unit directions only, so one of |c|, |s| is
// at least 0.7 while a float32 coordinate below 65536 has an ulp of at most 2^-8: every step moves the point at least
// ~0.7 px along one axis and the walk leaves the image within 1.5 * max(w, h) steps.  max_steps = 2 (w + h) + 4 caps
// it anyway; a ray that reaches the cap is counted (0 on every valid input).
//
// Latency: the positions along a ray do not depend on the pixels read, so a lane computes the next kRayAhead positions,
// issues their byte loads together (clamped into the image: a position past the border is never tested, the test of
// the one before it stops the ray) and then tests them in order -- one L2 / Infinity Cache round trip per kRayAhead
// steps instead of one per step (in the ISA: eight global_load_ubyte back to back, then vmcnt(7) .. vmcnt(0)).  Consecutive lanes are consecutive angles of one viewpoint: their first tens of
// pixels share cache lines.
#pragma once

namespace ym {

struct RayArgs {
    const uint8_t *img; // [height][pitch]
    int width, height, pitch;
    const double *starts; // [n_starts][2] pixel units
    const double *dirs;   // [n_angles][2] (cos, sin), or [n_starts][n_angles][2] when dirs_per_start
    int n_starts, n_angles;
    int dirs_per_start;
    int max_steps;
    float *end_xy;        // [n_starts][n_angles][2]
    double *length;       // [n_starts][n_angles]
    unsigned long long *capped;
};

constexpr int kRayAhead = 8;

// one thread per (viewpoint, angle) pair, flat index = viewpoint * n_angles + angle.  grid ceil(n / 256)
__global__ __launch_bounds__(256) void raytrace_kernel(RayArgs a) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned na = (unsigned)a.n_angles;
    if (t >= (unsigned)a.n_starts * na) return;
    const unsigned vp = t / na, ang = t - vp * na;
    const size_t d = a.dirs_per_start ? (size_t)t : ang;
    const double c = a.dirs[2 * d], s = a.dirs[2 * d + 1];
    const double jc = 1000.0 * c, js = 1000.0 * s;
    const float x0 = (float)a.starts[2 * vp], y0 = (float)a.starts[2 * vp + 1];
    const float xhi = (float)(a.width - 1), yhi = (float)(a.height - 1);
    float x = x0, y = y0;
    int steps = 0;
    bool run = true;
    while (run) {
        // positions px[0] (the current one, already admitted) .. px[kRayAhead]
        float px[kRayAhead + 1], py[kRayAhead + 1];
        px[0] = x; py[0] = y;
#pragma unroll
        for (int k = 1; k <= kRayAhead; k++) {
            px[k] = (float)((double)px[k - 1] + c);
            py[k] = (float)((double)py[k - 1] + s);
        }
        // the loads of all kRayAhead positions.  Left to itself the compiler sinks load k into the branch taken after step
        // k - 1's test (a chain of one memory round trip per step; folding the pixels into bit masks does not stop it, it
        // splits the masks again): the empty asm below takes every loaded value as an operand, so all eight loads are
        // issued back to back before the first test and waited for together
        unsigned v[kRayAhead];
#pragma unroll
        for (int k = 0; k < kRayAhead; k++) {
            const int xi = min(max((int)rintf(px[k]), 0), a.width - 1);
            const int yi = min(max((int)rintf(py[k]), 0), a.height - 1);
            v[k] = a.img[(size_t)yi * a.pitch + xi];
        }
#pragma unroll
        for (int k = 0; k < kRayAhead; k++) asm volatile("" : "+v"(v[k]));
#pragma unroll
        for (int k = 0; k < kRayAhead; k++) {
            float nx = px[k + 1], ny = py[k + 1];
            steps++;
            const bool hit = v[k] < 210u;
            if (hit && v[k] > 180u) { // "unknown": 180 < val < 210
                nx = (float)((double)nx + jc);
                ny = (float)((double)ny + js);
            }
            const float rx = rintf(nx), ry = rintf(ny);
            const bool out = ry < 1.0f || rx < 1.0f || rx >= xhi || ry >= yhi;
            x = nx; y = ny;
            if (hit || out) { run = false; break; }
            if (steps >= a.max_steps) {
                atomicAdd(a.capped, 1ull);
                run = false;
                break;
            }
        }
    }
    const float dx = x - x0, dy = y - y0; // RayInfo.length: (end - start).norm, the difference a float32 Point2
    reinterpret_cast<float2 *>(a.end_xy)[t] = make_float2(x, y);
    a.length[t] = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
}

}  // namespace ym
