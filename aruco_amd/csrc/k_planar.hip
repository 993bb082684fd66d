// Both planar pose solutions of every marker, batched (planar_device.h). Work mapping of pose_kernel (k_finalize.hip): four lanes share
// a marker, one corner each, butterfly sums inside the group of four, the small solves redundantly on every lane; sixteen markers per
// wave; a batch's markers come from the flat list finalize_kernel wrote.
#include "internal.h"
#include "planar_device.h"

namespace ah {

constexpr int PLANAR_G = 4;

// list != nullptr: the flat marker list of the first nframes frames a worker holds, marker i of its frame f goes to
// out[(first + f) * cap_out + i]; else markers[0 .. n_direct) go to out[0 .. n_direct)
__global__ __launch_bounds__(64) void planar_poses_kernel(const arucohip_marker_t* markers, const uint32_t* list, const uint32_t* counters,
                                                          uint32_t cap_list, int cap_markers, int n_direct, int nframes, int first, int cap_out,
                                                          CamModel cam, int refine, arucohip_planar_poses_t* out) {
    latency_bound_priority();
    __shared__ float s_obj[16][12], s_img[16][8];
    const int grp = threadIdx.x / PLANAR_G, sub = threadIdx.x % PLANAR_G;
    const uint32_t gid = blockIdx.x * (64 / PLANAR_G) + grp;
    const uint32_t n = list ? min(counters[CNT_NMARK], cap_list) : (uint32_t)n_direct;
    if (gid >= n) return;   // uniform within the group of four, as every exit below
    const arucohip_marker_t* m = markers + gid;
    arucohip_planar_poses_t* o = out + gid;
    if (list) {
        const uint32_t e = list[gid];
        const int f = (int)(e >> 16), i = (int)(e & 0xFFFFu);
        if (f >= nframes || i >= cap_out || i >= cap_markers) return;
        m = markers + (size_t)f * cap_markers + i;
        o = out + (size_t)(first + f) * cap_out + i;
    }
    const float hs = (float)((double)cam.marker_size / 2.);
    // getObjectPoints: (-,-), (-,+), (+,+), (+,-)
    float* obj = s_obj[grp];
    float* img = s_img[grp];
    obj[3 * sub] = (sub < 2) ? -hs : hs, obj[3 * sub + 1] = (sub == 1 || sub == 2) ? hs : -hs, obj[3 * sub + 2] = 0.f;
    img[2 * sub] = m->corners[2 * sub], img[2 * sub + 1] = m->corners[2 * sub + 1];
    double r0[3] = {0, 0, 0}, t0[3] = {0, 0, 0}, r1[3] = {0, 0, 0}, t1[3] = {0, 0, 0}, rms[2] = {0, 0};
    const int ns = planar_poses_wave<PLANAR_G>(obj, img, 4, cam, sub, refine != 0, r0, t0, r1, t1, rms);
    if (ns && cam.y_perp) rotate_x_axis(r0), rotate_x_axis(r1);
    if (sub == 0) {
        const bool ok = ns != 0;
        for (int k = 0; k < 3; k++) {
            o->rvec[0][k] = ok ? r0[k] : 0, o->rvec[1][k] = ok ? r1[k] : 0;
            o->tvec[0][k] = ok ? t0[k] : 0, o->tvec[1][k] = ok ? t1[k] : 0;
        }
        o->rms[0] = ok ? rms[0] : 0, o->rms[1] = ok ? rms[1] : 0;
        o->n_solutions = ns, o->pad_ = 0;
    }
}

void launch_planar_poses(hipStream_t s, const arucohip_marker_t* markers, int n, const CamModel& cam, int refine, arucohip_planar_poses_t* out) {
    hipLaunchKernelGGL(planar_poses_kernel, dim3((n + 15) / 16), dim3(64), 0, s, markers, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, 0, n, 0,
                       0, 0, cam, refine, out);
}

void launch_planar_poses_list(hipStream_t s, int list_frames, int nframes, int first, const Buffers& b, const CamModel& cam, int refine,
                              arucohip_planar_poses_t* out, int cap_out) {
    // the list's length is only known on the device and its order across frames is arbitrary: the grid covers the capacity of all
    // list_frames frames the worker detected, surplus workgroups and the markers of frames past nframes exit at once
    const uint32_t cap_list = (uint32_t)list_frames * (uint32_t)b.cap_markers;
    hipLaunchKernelGGL(planar_poses_kernel, dim3((cap_list + 15) / 16), dim3(64), 0, s, (const arucohip_marker_t*)b.markers, (const uint32_t*)b.marker_list,
                       (const uint32_t*)b.counters, cap_list, b.cap_markers, 0, nframes, first, cap_out, cam, refine, out);
}

}  // namespace ah
