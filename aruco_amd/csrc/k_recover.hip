// Board marker recovery: a board's markers that the decoder rejected are taken back from the frame's rejected candidates, on the lists the
// last batch left in HBM. No reference counterpart (ArUco 1.3 has none; OpenCV's aruco module calls it refineDetectedMarkers).
//
// Per frame, one 64-lane workgroup:
//   recover_match_kernel  : board pose from the frame's member markers (board_solve_wave, before rotateXAxis); for every board entry the frame
//                           lacks, in board order: project its four corners, take the free rejected candidate and cyclic rotation whose
//                           largest corner distance is smallest (lanes over candidates in trips of 64, wave argmin on (distance, index,
//                           rotation)), accept it below max_corner_dist when its 49 cell votes differ from the expected marker in at most
//                           max_cell_errors cells (49 lanes, ballot, popcount). An accepted candidate gets id and nrot.
//   (k_refine.hip)        : refine_one on the adopted candidates, as detection would have refined them.
//   recover_insert_kernel : border rectangle of finalize_kernel, insertion into the frame's marker list in id order, then the board is
//                           solved again over all members.
#include <algorithm>

#include "internal.h"
#include "decode_device.h"
#include "board_device.h"

namespace ah {

struct RecoverK {
    arucohip_marker_t* markers;
    int32_t* nmarkers;
    int cap_markers;
    Cand* cands;
    const int32_t* ncands;
    int cap_cands;
    const uint32_t* cand_list;
    uint32_t* counters;
    uint32_t* marker_list;
    uint32_t cap_flat;
    const int32_t* othr;
    const uint8_t* cells;
    const uint8_t* patches;
    RecoverArgs a;
    CamModel cam;
    RecoverBufs r;
    arucohip_board_t* boards;
    float* prob;
};

constexpr int RECOVER_MAX_CANDS = 512;   // = the largest candidates_per_frame arucohip_create_ex accepts

// base[f] = where frame f's block starts in the flat candidate list (frame_candidates_kernel appends a frame's candidates in one piece)
__global__ void recover_base_kernel(const uint32_t* cand_list, const uint32_t* counters, uint32_t cap_flat, int32_t* base, int nframes) {
    const uint32_t n = min(counters[CNT_NCAND], cap_flat);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t e = cand_list[i];
        if ((e & 0xFFFFu) == 0 && (int)(e >> 16) < nframes) base[e >> 16] = (int32_t)i;
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// the marker `id` as the decoders see it: bit cy * 7 + cx of the 7 x 7 grid, black border, row y of the code = the word its two id bits name
__device__ __forceinline__ unsigned long long fiducial_word(int id) {
    const unsigned long long words[4] = {0x01, 0x1D, 0x12, 0x0E};   // 10000, 10111, 01001, 01110, bit x = column x (hamm_rows)
    unsigned long long m = 0;
#pragma unroll
    for (int y = 0; y < 5; y++) m |= words[(id >> (2 * (4 - y))) & 3] << (7 * (y + 1) + 1);
    return m;
}

__global__ __launch_bounds__(64) void recover_match_kernel(RecoverK k) {
    latency_bound_priority();
    __shared__ BoardLds s;
    __shared__ float s_proj[8];
    __shared__ uint8_t s_taken[RECOVER_MAX_CANDS];
    const int frame = blockIdx.x, lane = threadIdx.x;
    const RecoverArgs& a = k.a;
    int nrec = 0;
    const int nm_raw = k.nmarkers[frame];
    const int nm = min(nm_raw, k.cap_markers);
    const int nc = min(min(k.ncands[frame], k.cap_cands), RECOVER_MAX_CANDS);
    double r[3], t[3];
    int nk = 0;
    const int st = nm_raw >= 0 ? board_solve_wave(k.markers + (size_t)frame * k.cap_markers, nm, a.bd, k.cam, k.counters, s, lane, r, t, &nk) : BOARD_NOT_TRIED;
    if (st == BOARD_POSE && nk >= a.min_markers && nc > 0) {
        const arucohip_marker_t* M = k.markers + (size_t)frame * k.cap_markers;
        Cand* C = k.cands + (size_t)frame * k.cap_cands;
        const uint32_t base = (uint32_t)k.r.base[frame];
        RecoverRec* rec = k.r.rec + (size_t)frame * k.cap_markers;
        uint32_t* rlist = k.r.rlist + (size_t)frame * k.cap_markers;
        for (int i = lane; i < nc; i += WAVE) s_taken[i] = 0;
        double R[9];
        rodrigues_vec2mat(r, R, nullptr);
        const double mpp = board_mpp(a.bd);
        __syncthreads();
        for (int j = 0; j < a.bd.nboard; j++) {
            const int want = a.bd.ids[j];
            bool have = false;
            for (int i = lane; i < nm; i += WAVE) have = have || M[i].id == want;
            if (__ballot(have)) continue;
            if (nm + nrec >= k.cap_markers) {   // the frame's marker list is full: recovery stops here, the call reports it
                if (lane == 0) atomicOr(k.r.status, 1u);
                break;
            }
            __syncthreads();   // the previous entry's readers of s_proj are done
            if (lane < 4) {
                const float* q = a.bd.obj + ((size_t)j * 4 + lane) * 3;
                double mx, my;
                project_point((float)(q[0] * mpp), (float)(q[1] * mpp), (float)(q[2] * mpp), R, nullptr, t, k.cam.K, k.cam.k, &mx, &my, nullptr, nullptr);
                s_proj[2 * lane] = (float)mx, s_proj[2 * lane + 1] = (float)my;
            }
            __syncthreads();
            // (largest corner distance, candidate, rotation): rotation rot pairs projected corner i with quad corner (i + 4 - rot) & 3, the
            // decoders' nRotations
            unsigned long long best = ~0ull;
            for (int c0 = 0; c0 < nc; c0 += WAVE) {
                const int ci = c0 + lane;
                if (ci >= nc || C[ci].id != -1 || s_taken[ci]) continue;
                float d[4][4];   // [quad corner][projected corner]
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const float ex = (float)C[ci].qx[q] - s_proj[2 * p], ey = (float)C[ci].qy[q] - s_proj[2 * p + 1];
                        d[q][p] = (float)sqrt((double)ex * ex + (double)ey * ey);
                    }
#pragma unroll
                for (int rot = 0; rot < 4; rot++) {
                    float dm = 0.f;
#pragma unroll
                    for (int p = 0; p < 4; p++) dm = fmaxf(dm, d[(p + 4 - rot) & 3][p]);
                    const unsigned long long key = ((unsigned long long)__float_as_uint(dm) << 32) | (unsigned long long)(ci << 2 | rot);
                    best = key < best ? key : best;
                }
            }
            best = wave_min_u64(best);
            if (best == ~0ull) continue;
            const float dist = __uint_as_float((uint32_t)(best >> 32));
            if (!(dist < a.max_corner_dist)) continue;
            const int ci = (int)((best >> 2) & 0x3FFFFFFFu), rot = (int)(best & 3u);
            const uint32_t li = base + (uint32_t)ci;
            // the flat list overflowed (the frame is given up anyway): the candidate was never warped
            if (k.r.base[frame] < 0 || li >= k.cap_flat || k.cand_list[li] != (((uint32_t)frame << 16) | (uint32_t)ci)) continue;
            // the candidate's 49 cell votes, bit cy * 7 + cx
            const int thr = k.othr[li];
            unsigned long long m;
            if (a.cells_valid) {
                bool white = false;
                if (lane < 49) white = (int)k.cells[(size_t)li * 64 + (lane / 7) * CELLS_PITCH + lane % 7] > thr;
                m = __ballot(white);
            } else {
                m = cells_votes_wave(k.patches + (size_t)li * a.ws * a.ws, a.ws, thr, lane);
            }
            // turned rot times as fiducial_decode_word turns the code (new[i][j] = old[n - 1 - j][i]), then held against the expected marker
            bool bit = false;
            if (lane < 49) {
                int i = lane / 7, jj = lane % 7;
                for (int q = 0; q < rot; q++) {
                    const int si = 6 - jj, sj = i;
                    i = si, jj = sj;
                }
                bit = (m >> (i * 7 + jj)) & 1ull;
            }
            const unsigned long long mr = __ballot(bit);
            const int errors = __popcll(mr ^ fiducial_word(want));
            if (errors > a.max_cell_errors) continue;
            if (lane == 0) {
                RecoverRec e;
                e.board = j, e.cand = ci, e.nrot = rot, e.old_nrot = C[ci].nrot;
                rec[nrec] = e;
                rlist[nrec] = ((uint32_t)frame << 16) | (uint32_t)ci;
                C[ci].id = want, C[ci].nrot = rot;
                s_taken[ci] = 1;
            }
            nrec++;
        }
    }
    if (lane == 0) k.r.nrec[frame] = nrec;
}

__global__ __launch_bounds__(64) void recover_insert_kernel(RecoverK k) {
    latency_bound_priority();
    __shared__ BoardLds s;
    __shared__ int s_nm;
    const int frame = blockIdx.x, lane = threadIdx.x;
    const RecoverArgs& a = k.a;
    arucohip_marker_t* M = k.markers + (size_t)frame * k.cap_markers;
    uint32_t* plist = k.r.plist + (size_t)frame * k.cap_markers;
    for (int i = lane; i < k.cap_markers; i += WAVE) plist[i] = 0xFFFFFFFFu;
    __syncthreads();
    if (lane == 0) {
        const int nrec = k.r.nrec[frame];
        const int nm0 = min(k.nmarkers[frame], k.cap_markers);
        int nm = nm0;
        Cand* C = k.cands + (size_t)frame * k.cap_cands;
        const RecoverRec* rec = k.r.rec + (size_t)frame * k.cap_markers;
        for (int q = 0; q < nrec; q++) {
            Cand* cand = C + rec[q].cand;
            bool inside = true;
            for (int c = 0; c < 4; c++) {   // finalize_kernel's border filter
                const int px = __float2int_rn(cand->c[2 * c]), py = __float2int_rn(cand->c[2 * c + 1]);
                inside = inside && a.bx0 <= px && px < a.bx1 && a.by0 <= py && py < a.by1;
            }
            if (!inside || nm >= k.cap_markers) {   // not adopted: the candidate is a rejected one again, as frame_candidates_kernel left it
                cand->id = -1, cand->nrot = rec[q].old_nrot;
                for (int c = 0; c < 4; c++) cand->c[2 * c] = (float)cand->qx[c], cand->c[2 * c + 1] = (float)cand->qy[c];
                continue;
            }
            arucohip_marker_t m;
            m.id = cand->id;
            for (int c = 0; c < 8; c++) m.corners[c] = cand->c[c];
            m.ssize = -1.f, m.has_pose = 0, m.pad_ = 0;
            for (int c = 0; c < 3; c++) m.rvec[c] = m.tvec[c] = 0;
            int at = nm;   // behind the markers of smaller or equal id
            while (at > 0 && M[at - 1].id > m.id) M[at] = M[at - 1], at--;
            M[at] = m;
            nm++;
        }
        const int kept = nm - nm0;
        if (kept > 0) {
            int w = 0;   // where the adopted ones went: their ids were missing from the frame, so each is found once
            for (int q = 0; q < nrec; q++) {
                const int id = C[rec[q].cand].id;
                if (id < 0) continue;
                for (int i = 0; i < nm; i++)
                    if (M[i].id == id) {
                        plist[w++] = ((uint32_t)frame << 16) | (uint32_t)i;
                        break;
                    }
            }
            k.nmarkers[frame] = nm;
            // the batch's flat marker list names slots, not markers: the new slots join it (planar poses walk it)
            const uint32_t base = atomicAdd(&k.counters[CNT_NMARK], (uint32_t)kept);
            for (int i = 0; i < kept; i++) k.marker_list[base + i] = ((uint32_t)frame << 16) | (uint32_t)(nm0 + i);
        }
        k.r.recovered[frame] = kept;
        s_nm = nm;
    }
    __threadfence_block();
    __syncthreads();
    // the board over all members, as board_pose_kernel gives it
    double r[3], t[3];
    int nk;
    const int st = board_solve_wave(M, max(s_nm, 0), a.bd, k.cam, k.counters, s, lane, r, t, &nk);
    arucohip_board_t res;
    res.n_markers = nk, res.has_pose = 0;
    for (int c = 0; c < 3; c++) res.rvec[c] = res.tvec[c] = 0;
    float prob = 0;
    if (st != BOARD_NOT_TRIED) {
        if (st == BOARD_POSE && k.cam.y_perp) rotate_x_axis(r);
        res.has_pose = st == BOARD_POSE ? 1 : 0;
        for (int c = 0; c < 3; c++) res.rvec[c] = r[c], res.tvec[c] = t[c];
        prob = (float)nk / (float)a.bd.nboard;
    }
    if (lane == 0) k.boards[frame] = res, k.prob[frame] = prob;
}

static RecoverK recover_args(const Buffers& b, const RecoverArgs& a, const CamModel& cam, const RecoverBufs& r) {
    RecoverK k;
    k.markers = b.markers, k.nmarkers = b.nmarkers, k.cap_markers = b.cap_markers;
    k.cands = b.cands, k.ncands = b.ncands, k.cap_cands = b.cap_cands;
    k.cand_list = b.cand_list, k.counters = b.counters, k.marker_list = b.marker_list, k.cap_flat = b.cap_flat;
    k.othr = b.othr, k.cells = b.cells, k.patches = b.patches;
    k.a = a, k.cam = cam, k.r = r, k.boards = nullptr, k.prob = nullptr;
    return k;
}

// list_frames: the frames the worker's flat candidate list covers (its whole chunk); nframes <= list_frames: the frames to work on
void launch_recover_match(hipStream_t s, int list_frames, int nframes, const Buffers& b, const RecoverArgs& a, const CamModel& cam, const RecoverBufs& r) {
    const uint32_t cap_list = std::min<uint32_t>(b.cap_flat, (uint32_t)list_frames * (uint32_t)b.cap_cands);
    hipLaunchKernelGGL(recover_base_kernel, dim3(std::max(1u, std::min((cap_list + 255u) / 256u, 256u))), dim3(256), 0, s, (const uint32_t*)b.cand_list,
                       (const uint32_t*)b.counters, b.cap_flat, r.base, nframes);
    hipLaunchKernelGGL(recover_match_kernel, dim3(nframes), dim3(64), 0, s, recover_args(b, a, cam, r));
}

void launch_recover_insert(hipStream_t s, int nframes, const Buffers& b, const RecoverArgs& a, const CamModel& cam, const RecoverBufs& r,
                           arucohip_board_t* boards, float* prob) {
    RecoverK k = recover_args(b, a, cam, r);
    k.boards = boards, k.prob = prob;
    hipLaunchKernelGGL(recover_insert_kernel, dim3(nframes), dim3(64), 0, s, k);
}

}  // namespace ah
