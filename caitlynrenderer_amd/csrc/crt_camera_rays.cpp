// The caller's own camera rays (include/crt.h at crt_set_camera_rays): the three entries and the life of the buffer they
// fill.  What a frame makes of the rays is crt_frames.cpp's (FramePlan::rays, launch_primary_rays) and rt_kernels.hip's (k_raygen_rays).
#include "crt_scene.hpp"

using crt::dev_alloc;
using crt::fail;

namespace {

// every stream of the scene drains: a frame enqueued earlier keeps the rays it was enqueued with (option "streams": the replicas read the
// same buffer on streams of their own)
int drain(crt_scene* s) {
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (crt_scene* p : s->peers) HIPCHK(hipStreamSynchronize(p->stream));
    return CRT_OK;
}

int set_rays(crt_scene* s, const void* rays, size_t n, bool on_device, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    if (!s) return fail(CRT_ERR_INVALID, who + "null scene");
    if (!rays) return fail(CRT_ERR_INVALID, who + "rays is null");
    if (s->primary) return fail(CRT_ERR_INVALID, who + "not on a replica");
    if (n != (size_t)s->width * s->height) return fail(CRT_ERR_INVALID, who + "n must be width * height, one entry per pixel");
    if (!s->peers.empty() && s->streams <= 1u)
        return fail(CRT_ERR_INVALID, who + "devices: a scene on several devices (crt_set_devices) takes no camera rays");
    int rc = drain(s);
    if (rc) return rc;
    float4* buf = s->d_cam_rays;
    if (!buf && (rc = dev_alloc(&buf, 2 * n))) return rc;
    const hipError_t e = hipMemcpyAsync(buf, rays, n * sizeof(crt_ray), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream);
    if (e != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
        // the buffer may hold part of the new set: with no earlier set nothing is lost, and an earlier one can no longer be vouched for
        if (!s->d_cam_rays) (void)hipFree(buf);
        else s->cam_rays_set = false;
        (void)hipGetLastError();
        return fail(CRT_ERR_HIP, who + "copying the rays failed");
    }
    s->d_cam_rays = buf;
    s->cam_rays_set = true;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_set_camera_rays(crt_scene* s, const crt_ray* rays, size_t n) { return set_rays(s, rays, n, false, "crt_set_camera_rays"); }

int crt_set_camera_rays_device(crt_scene* s, const void* d_rays, size_t n) { return set_rays(s, d_rays, n, true, "crt_set_camera_rays_device"); }

int crt_clear_camera_rays(crt_scene* s) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_clear_camera_rays: null scene");
    if (s->primary) return fail(CRT_ERR_INVALID, "crt_clear_camera_rays: not on a replica");
    const int rc = drain(s);
    if (rc) return rc;
    s->cam_rays_set = false;             // the buffer stays for the next set
    return CRT_OK;
}

}  // extern "C"
