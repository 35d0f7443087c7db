// ym_abi_rays.hpp -- C ABI: virtual scans ray-traced from an occupancy image (ym_raymap_*; ym_k_raytrace.hpp)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
struct ym_raymap {
    int device;
    int width, height;   // the image, resident on the device with pitch = width
    OwnStream stream;
    DevBuf<uint8_t> d_img;
    DevBuf<double> starts, dirs, length;
    DevBuf<float> end_xy;
    DevBuf<unsigned long long> capped;
};

ym_raymap *ym_raymap_create(int device, const uint8_t *image, int width, int height, int pitch) {
    if (!image || width < 1 || height < 1 || pitch < width) { set_err(YM_ERR_INVALID, "bad occupancy image"); return nullptr; }
    if (width > 65536 || height > 65536) {
        set_err(YM_ERR_INVALID, "image of %d x %d pixels: at most 65536 x 65536 (the walk's termination bound)", width, height);
        return nullptr;
    }
    if (check_device(device) != YM_OK) return nullptr;
    DevGuard guard(device);
    if (guard.status() != YM_OK) return nullptr;
    ym_raymap *rm = new ym_raymap();
    rm->device = device; rm->width = width; rm->height = height;
    auto setup = [&]() -> int {
        int rc;
        if ((rc = rm->stream.create()) || (rc = rm->d_img.alloc((size_t)width * height))) return rc;
        HIP_TRY(hipMemcpy2D(rm->d_img.p, width, image, pitch, width, height, hipMemcpyHostToDevice));
        return YM_OK;
    };
    if (setup() != YM_OK) { delete rm; return nullptr; } // (the error text is set)
    return rm;
}

static int raymap_trace(ym_raymap *rm, const double *starts_xy, int n_starts, const double *dir_cs, int n_angles, bool per_start,
                        float *end_xy, double *length, int64_t *capped) {
    if (!rm) return set_err(YM_ERR_INVALID, "null raymap");
    if (n_starts < 0 || n_angles < 0) return set_err(YM_ERR_INVALID, "negative count");
    if (n_starts == 0 || n_angles == 0) {
        if (capped) *capped = 0;
        return YM_OK;
    }
    if (!starts_xy || !dir_cs || !end_xy || !length) return set_err(YM_ERR_INVALID, "null argument");
    const int64_t n = (int64_t)n_starts * n_angles;
    if (n > (int64_t)INT32_MAX - 255) return set_err(YM_ERR_INVALID, "%lld rays in one call: at most 2^31 - 256", (long long)n);
    // the first read is at the start pixel, before the walk's bounds test (in numba, an out-of-bounds read)
    for (int i = 0; i < n_starts; i++) {
        const double sx = starts_xy[2 * i], sy = starts_xy[2 * i + 1];
        if (!std::isfinite(sx) || !std::isfinite(sy))
            return set_err(YM_ERR_INVALID, "start %d is not finite", i);
        const float xr = std::nearbyint((float)sx), yr = std::nearbyint((float)sy);
        if (xr < 0.0f || yr < 0.0f || xr > (float)(rm->width - 1) || yr > (float)(rm->height - 1))
            return set_err(YM_ERR_INVALID, "start %d (%g, %g) rounds to a pixel outside the %d x %d image", i, sx, sy, rm->width,
                           rm->height);
    }
    // unit directions: the termination bound needs one of |c|, |s| >= 0.7
    const int64_t n_dirs = per_start ? n : n_angles;
    for (int64_t k = 0; k < n_dirs; k++) {
        const double c = dir_cs[2 * k], s = dir_cs[2 * k + 1];
        if (!(std::fabs(c * c + s * s - 1.0) <= 1e-9)) return set_err(YM_ERR_INVALID, "direction %lld (%g, %g) is not a unit vector", (long long)k, c, s);
    }
    DEV_GUARD(rm->device);
    int rc;
    if ((rc = rm->starts.ensure(2 * (size_t)n_starts)) || (rc = rm->dirs.ensure(2 * (size_t)n_dirs)) ||
        (rc = rm->end_xy.ensure(2 * (size_t)n)) || (rc = rm->length.ensure((size_t)n)) || (rc = rm->capped.ensure(1)))
        return rc;
    HIP_TRY(hipMemcpyAsync(rm->starts.p, starts_xy, sizeof(double) * 2 * n_starts, hipMemcpyHostToDevice, rm->stream));
    HIP_TRY(hipMemcpyAsync(rm->dirs.p, dir_cs, sizeof(double) * 2 * n_dirs, hipMemcpyHostToDevice, rm->stream));
    HIP_TRY(hipMemsetAsync(rm->capped.p, 0, sizeof(unsigned long long), rm->stream));
    ym::RayArgs a;
    a.img = rm->d_img.p; a.width = rm->width; a.height = rm->height; a.pitch = rm->width;
    a.starts = rm->starts.p; a.dirs = rm->dirs.p; a.n_starts = n_starts; a.n_angles = n_angles;
    a.dirs_per_start = per_start ? 1 : 0;
    a.max_steps = 2 * (rm->width + rm->height) + 4;
    a.end_xy = rm->end_xy.p; a.length = rm->length.p; a.capped = rm->capped.p;
    hipLaunchKernelGGL(ym::raytrace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, rm->stream, a);
    HIP_TRY(hipGetLastError());
    unsigned long long n_capped = 0;
    HIP_TRY(hipStreamSynchronize(rm->stream));
    // (the outputs are written only once the whole trace has succeeded)
    HIP_TRY(hipMemcpy(&n_capped, rm->capped.p, sizeof n_capped, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(end_xy, rm->end_xy.p, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(length, rm->length.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (capped) *capped = (int64_t)n_capped;
    return YM_OK;
}

int ym_raymap_trace(ym_raymap *rm, const double *starts_xy, int n_starts, const double *dir_cs, int n_angles, float *end_xy,
                    double *length, int64_t *capped) {
    return raymap_trace(rm, starts_xy, n_starts, dir_cs, n_angles, false, end_xy, length, capped);
}

int ym_raymap_trace_each(ym_raymap *rm, const double *starts_xy, int n_starts, const double *dir_cs, int n_angles, float *end_xy,
                         double *length, int64_t *capped) {
    return raymap_trace(rm, starts_xy, n_starts, dir_cs, n_angles, true, end_xy, length, capped);
}

void ym_raymap_destroy(ym_raymap *rm) {
    if (!rm) return;
    DevGuard guard(rm->device);
    delete rm;
}
