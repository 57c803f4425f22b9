// track_pose.hip -- the pose bookkeeping of the tracking thread and the trajectory read-out, on resident arrays, on gfx950.
//
// Restates (thirdparty/orb-slam2):
//   Tracking::UpdateLastFrame, the monocular return      src/Tracking.cc:792-798
//   TrackWithMotionModel / TrackReferenceKeyFrame's pose :866 / :764
//   Tracking::Track, motion model, mLastFrame, the record :432-440, :493, :497-506
//   KeyFrame::SetBadFlag's mTcp                          src/KeyFrame.cc:641
//   System::GetTrajectory                                src/System.cc:371-412
// under the readings of DESIGN.md section 4; every one of them is a single copy in loop_pose.h, g2o_se3.h or g2o_lm.h: lp_mul44 (the 4 x 4
// float product), lp_twc (GetPoseInverse), po_set_ow (SetPose's Ow, and -rotation_mat * t of GetTrajectory, which is the same
// expression), g2o_quat_from_matrix (Converter::toEigenQuaternion).
//   k_tp_predict   a thread per tracker
//   k_tp_commit    a thread per tracker
//   k_tp_tcp       a thread per record of a key-frame culling
//   k_traj_origin  one workgroup: the live key frame of smallest (mnId, index), into info[1]
//   k_traj_records a thread per record; the walk up the culled key frames is bounded by nkf steps
// Integer atomics only count; no floating-point atomic, no scratch arena.
#include "loop_pose.h"
#include <math.h>
#include <string>
#include <vector>

#define TP_T 256

static_assert(sizeof(pgorb_kf_pose) == 84 && sizeof(pgorb_track_state) == 140 && sizeof(pgorb_trajectory_record) == 72, "record layouts");

__device__ __forceinline__ void tp_set(float* dst, const float (&src)[12])
{
#pragma unroll
    for (int q = 0; q < 12; q++) dst[q] = src[q];
}

struct TpArgs {
    int ntrack, mode; const int32_t* modes; pgorb_track_state* state; pgorb_trajectory_record* traj; int cap; int32_t* ntraj;
    int nkf; const pgorb_kf_pose* kfPose; const pgorb_kf_pose* pose; const uint8_t* ok; const int32_t* refKf; const double* time;
    const int64_t* id; pgorb_kf_pose* poseOut; int32_t* status;
};

__global__ __launch_bounds__(TP_T) void k_tp_predict(TpArgs A)
{
    const int t = blockIdx.x * TP_T + threadIdx.x;
    if (t >= A.ntrack) return;
    pgorb_track_state st = A.state[t];
    const int m = A.modes ? A.modes[t] : A.mode;
    const int cnt = A.ntraj ? A.ntraj[t] : 0;
    int status = st.has_last ? 0 : PGORB_TRACK_NO_LAST;
    if (m == PGORB_TRACK_MOTION_MODEL) {
        if (!st.has_velocity) status |= PGORB_TRACK_NO_VELOCITY;
        if (st.last_ref_kf < 0 || st.last_ref_kf >= A.nkf || cnt < 1 || cnt > A.cap || !A.traj[(int64_t)t * A.cap + cnt - 1].has_pose)
            status |= PGORB_TRACK_BAD_INDEX;
    } else if (m != PGORB_TRACK_REFERENCE_KF) status |= PGORB_TRACK_BAD_INDEX;
    A.status[t] = status;
    pgorb_kf_pose o = st.last;
    if (!status && m == PGORB_TRACK_MOTION_MODEL) {
        float T[12];
        lp_mul44(A.traj[(int64_t)t * A.cap + cnt - 1].pose, A.kfPose[st.last_ref_kf].Tcw, T);   // Tlr*pRef->GetPose() (:798)
        tp_set(st.last.Tcw, T);
        po_set_ow(st.last);
        A.state[t].last = st.last;
        lp_mul44(st.velocity, st.last.Tcw, T);                                                  // mVelocity*mLastFrame.mTcw (:866)
        tp_set(o.Tcw, T);
        po_set_ow(o);
    }
    A.poseOut[t] = o;
}

__global__ __launch_bounds__(TP_T) void k_tp_commit(TpArgs A)
{
    const int t = blockIdx.x * TP_T + threadIdx.x;
    if (t >= A.ntrack) return;
    const int cnt = A.ntraj[t], ref = A.refKf[t];
    const int status = ((cnt < 0 || cnt >= A.cap) ? PGORB_TRACK_FULL : 0) | ((ref < 0 || ref >= A.nkf) ? PGORB_TRACK_BAD_INDEX : 0);
    A.status[t] = status;
    if (status) return;
    pgorb_track_state st = A.state[t];
    const pgorb_kf_pose P = A.pose[t];
    const bool ok = A.ok[t] != 0;
    float Twc[12], T[12];
    if (ok) {                                                                                   // :432-440
        if (st.has_last) {
            lp_twc(st.last, Twc);                                                               // GetRotationInverse(), GetCameraCenter()
            lp_mul44(P.Tcw, Twc, T);                                                            // mCurrentFrame.mTcw*LastTwc
            tp_set(st.velocity, T);
            st.has_velocity = 1;
        } else {
#pragma unroll
            for (int q = 0; q < 12; q++) st.velocity[q] = 0.f;
            st.has_velocity = 0;
        }
    }
    pgorb_trajectory_record R;                                                                  // :497-506
    lp_twc(A.kfPose[ref], Twc);
    lp_mul44(P.Tcw, Twc, T);
    tp_set(R.pose, T);
    R.ref_kf = ref; R.has_pose = 1; R.lost = ok ? 0 : 1; R.pad[0] = R.pad[1] = 0;
    R.frame_time = A.time[t]; R.frame_id = A.id[t];
    A.traj[(int64_t)t * A.cap + cnt] = R;
    A.ntraj[t] = cnt + 1;
    st.last = P; st.has_last = 1; st.last_ref_kf = ref;                                         // mLastFrame = Frame(mCurrentFrame) (:493)
    A.state[t] = st;
}

__global__ __launch_bounds__(TP_T) void k_tp_tcp(int nframes, const pgorb_kf_pose* pose, const int32_t* parent, int listCap,
                                                const int32_t* record, const int32_t* cullInfo, float* tcp, int32_t* info)
{
    const int g = blockIdx.x * TP_T + threadIdx.x;
    if (cullInfo[0] & PGORB_CULL_LIMIT) return;
    if (g >= min(max(cullInfo[1], 0), listCap) || record[g * 4 + 3] != PGORB_CULL_KF_CULLED) return;
    const int a = record[g * 4];
    const int p = (a >= 0 && a < nframes) ? parent[a] : -1;
    if (p < 0 || p >= nframes) { atomicAdd(&info[2], 1); return; }
    float Twc[12], T[12];
    lp_twc(pose[p], Twc);
    lp_mul44(pose[a].Tcw, Twc, T);                                                              // Tcw*mpParent->GetPoseInverse() (KeyFrame.cc:641)
    tp_set(tcp + (int64_t)a * 12, T);
    atomicAdd(&info[1], 1);
}

struct TrajArgs {
    int nkf; const pgorb_kf_pose* pose; const uint8_t* kfBad; const int32_t* parent; const uint64_t* kfId; const float* tcp;
    int n; const pgorb_trajectory_record* traj; const int32_t* count;
    double* quat; double* trans; int64_t* timeUsec; int64_t* frameId; uint8_t* isLost; int32_t* status; int32_t* info;
};

__global__ __launch_bounds__(TP_T) void k_traj_origin(TrajArgs A)
{
    __shared__ uint64_t sId[TP_T];
    __shared__ int sIdx[TP_T];
    uint64_t id = 0;
    int idx = -1;
    for (int k = threadIdx.x; k < A.nkf; k += TP_T)                                             // ascending k: the smaller index wins a tie
        if (!A.kfBad[k] && (idx < 0 || A.kfId[k] < id)) { id = A.kfId[k]; idx = k; }
    sId[threadIdx.x] = id; sIdx[threadIdx.x] = idx;
    __syncthreads();
    for (int h = TP_T / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const int j = sIdx[threadIdx.x + h], i = sIdx[threadIdx.x];
            const uint64_t dj = sId[threadIdx.x + h], di = sId[threadIdx.x];
            if (j >= 0 && (i < 0 || dj < di || (dj == di && j < i))) { sId[threadIdx.x] = dj; sIdx[threadIdx.x] = j; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        A.info[0] = sIdx[0] < 0 ? PGORB_TRAJ_NO_ORIGIN : 0;
        A.info[1] = sIdx[0];
        A.info[2] = 0;
        A.info[3] = A.count ? min(max(*A.count, 0), A.n) : A.n;
    }
}

__global__ __launch_bounds__(TP_T) void k_traj_records(TrajArgs A)
{
    const int i = blockIdx.x * TP_T + threadIdx.x;
    const int origin = A.info[1];
    if (origin < 0 || i >= A.info[3]) return;
    const pgorb_trajectory_record R = A.traj[i];
    int status = 0;
    const double us = __dmul_rn(R.frame_time, 1e6);                                             // static_cast<int64>(mFrameTime*1e6) (:386)
    int64_t tu;
    if (us >= -9223372036854775808.0 && us < 9223372036854775808.0) tu = (int64_t)us;
    else { tu = INT64_MIN; status |= PGORB_TRAJ_BAD_TIME; }
    A.timeUsec[i] = tu; A.frameId[i] = R.frame_id; A.isLost[i] = R.lost ? 1 : 0;
    double out[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!R.lost) {
        bool okay = R.has_pose != 0;
        float Trw[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f}, T[12];     // cv::Mat::eye(4, 4, CV_32F) (:394)
        int k = R.ref_kf;
        for (int steps = 0; okay; steps++) {                                                    // :397-400
            if (k < 0 || k >= A.nkf || steps >= A.nkf) { okay = false; break; }
            if (!A.kfBad[k]) break;
            lp_mul44(Trw, A.tcp + (int64_t)k * 12, T);
            tp_set(Trw, T);
            k = A.parent[k];
        }
        if (okay) {
            float Two[12], U[12];
            pgorb_kf_pose F;
            lp_twc(A.pose[origin], Two);
            lp_mul44(Trw, A.pose[k].Tcw, T);                                                    // Trw*pKF->GetPose()*Two (:402)
            lp_mul44(T, Two, U);
            lp_mul44(R.pose, U, F.Tcw);                                                         // mRelativeFramePose*Trw (:404)
            const double Rt[9] = {(double)F.Tcw[0], (double)F.Tcw[4], (double)F.Tcw[8], (double)F.Tcw[1], (double)F.Tcw[5], (double)F.Tcw[9],
                                  (double)F.Tcw[2], (double)F.Tcw[6], (double)F.Tcw[10]};       // rotation_mat = the block's .t() (:405)
            OsSim Q;
            g2o_quat_from_matrix(Rt, Q);
            po_set_ow(F);                                                                       // -rotation_mat*Tcw.col(3) (:407)
            out[0] = Q.qw; out[1] = Q.qx; out[2] = Q.qy; out[3] = Q.qz;
            out[4] = (double)F.Ow[0]; out[5] = (double)F.Ow[1]; out[6] = (double)F.Ow[2];
        } else {
            status |= PGORB_TRAJ_BROKEN;
            atomicAdd(&A.info[2], 1);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) A.quat[(int64_t)i * 4 + q] = out[q];
#pragma unroll
    for (int q = 0; q < 3; q++) A.trans[(int64_t)i * 3 + q] = out[4 + q];
    A.status[i] = status;
}

static inline unsigned tp_blocks(int n) { return (unsigned)((n + TP_T - 1) / TP_T); }

extern "C" {

int pgorb_track_predict_batch_device(pgorb_ctx* c, int ntrack, int mode, const int32_t* d_mode, pgorb_track_state* d_state,
        const pgorb_trajectory_record* d_traj, int traj_cap, const int32_t* d_ntrajectory, int nkf, const pgorb_kf_pose* d_kf_pose,
        pgorb_kf_pose* d_pose_out, int32_t* d_status, void* stream)
{
    if (!c) return PGORB_E_ARG;
    const bool motion = d_mode || mode == PGORB_TRACK_MOTION_MODEL;
    if (ntrack < 0 || nkf < 0 || traj_cap < 0 || (!d_mode && mode != PGORB_TRACK_MOTION_MODEL && mode != PGORB_TRACK_REFERENCE_KF) ||
        (ntrack && (!d_state || !d_pose_out || !d_status || (motion && (!d_ntrajectory || (traj_cap && !d_traj) || (nkf && !d_kf_pose))))))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_track_predict_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nkf > PGORB_COVIS_MAX_KF || traj_cap > PGORB_TRAJ_MAX_RECORDS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_track_predict: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    if (!ntrack) return 0;
    TpArgs A;
    memset(&A, 0, sizeof(A));
    A.ntrack = ntrack; A.mode = mode; A.modes = d_mode; A.state = d_state; A.traj = const_cast<pgorb_trajectory_record*>(d_traj); A.cap = traj_cap;
    A.ntraj = const_cast<int32_t*>(d_ntrajectory); A.nkf = nkf; A.kfPose = d_kf_pose; A.poseOut = d_pose_out; A.status = d_status;
    hipLaunchKernelGGL(k_tp_predict, dim3(tp_blocks(ntrack)), dim3(TP_T), 0, (hipStream_t)stream, A);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_tp_predict launch failed");
    return 0;
}

int pgorb_track_commit_batch_device(pgorb_ctx* c, int ntrack, pgorb_track_state* d_state, const pgorb_kf_pose* d_pose, const uint8_t* d_ok,
        const int32_t* d_ref_kf, const double* d_frame_time, const int64_t* d_frame_id, int nkf, const pgorb_kf_pose* d_kf_pose,
        pgorb_trajectory_record* d_traj, int traj_cap, int32_t* d_ntrajectory, int32_t* d_status, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (ntrack < 0 || nkf < 0 || traj_cap < 0 ||
        (ntrack && (!d_state || !d_pose || !d_ok || !d_ref_kf || !d_frame_time || !d_frame_id || !d_ntrajectory || !d_status ||
                    (traj_cap && !d_traj) || (nkf && !d_kf_pose))))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_track_commit_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nkf > PGORB_COVIS_MAX_KF || traj_cap > PGORB_TRAJ_MAX_RECORDS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_track_commit: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    if (!ntrack) return 0;
    TpArgs A;
    memset(&A, 0, sizeof(A));
    A.ntrack = ntrack; A.state = d_state; A.traj = d_traj; A.cap = traj_cap; A.ntraj = d_ntrajectory; A.nkf = nkf; A.kfPose = d_kf_pose;
    A.pose = d_pose; A.ok = d_ok; A.refKf = d_ref_kf; A.time = d_frame_time; A.id = d_frame_id; A.status = d_status;
    hipLaunchKernelGGL(k_tp_commit, dim3(tp_blocks(ntrack)), dim3(TP_T), 0, (hipStream_t)stream, A);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_tp_commit launch failed");
    return 0;
}

int pgorb_keyframe_tcp_device(pgorb_ctx* c, int nframes, const pgorb_kf_pose* d_pose, const int32_t* d_parent, int list_cap,
        const int32_t* d_record, const int32_t* d_cull_info, float* d_tcp, int32_t* d_info_out, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || list_cap < 0 || !d_info_out || (list_cap && (!d_record || !d_cull_info)) || (nframes && (!d_pose || !d_parent || !d_tcp)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_keyframe_tcp_device");
    if (nframes > PGORB_COVIS_MAX_KF || list_cap > PGORB_COVIS_MAX_KF)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_keyframe_tcp: more than PGORB_COVIS_MAX_KF key frames or records");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_info_out, 0, PGORB_TCP_INFO * 4, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (list_cap) hipLaunchKernelGGL(k_tp_tcp, dim3(tp_blocks(list_cap)), dim3(TP_T), 0, s, nframes, d_pose, d_parent, list_cap, d_record, d_cull_info, d_tcp, d_info_out);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_tp_tcp launch failed");
    return 0;
}

int pgorb_get_trajectory_device(pgorb_ctx* c, int nkf, const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, const int32_t* d_parent,
        const uint64_t* d_kf_id, const float* d_tcp, int n, const pgorb_trajectory_record* d_traj, const int32_t* d_count,
        double* d_quat_wxyz, double* d_translation, int64_t* d_time_usec, int64_t* d_frame_id, uint8_t* d_is_lost, int32_t* d_status,
        int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nkf < 0 || n < 0 || !d_info || (nkf && (!d_pose || !d_kf_bad || !d_parent || !d_kf_id || !d_tcp)) ||
        (n && (!d_traj || !d_quat_wxyz || !d_translation || !d_time_usec || !d_frame_id || !d_is_lost || !d_status)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_get_trajectory_device");
    if (nkf > PGORB_COVIS_MAX_KF || n > PGORB_TRAJ_MAX_RECORDS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_get_trajectory: more than PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const TrajArgs A = {nkf, d_pose, d_kf_bad, d_parent, d_kf_id, d_tcp, n, d_traj, d_count, d_quat_wxyz, d_translation, d_time_usec, d_frame_id,
                        d_is_lost, d_status, d_info};
    hipLaunchKernelGGL(k_traj_origin, dim3(1), dim3(TP_T), 0, s, A);
    if (n) hipLaunchKernelGGL(k_traj_records, dim3(tp_blocks(n)), dim3(TP_T), 0, s, A);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_traj_origin / k_traj_records launch failed");
    return 0;
}

// ---- the host forms: checked, then one synchronous call of the device form
int pgorb_track_predict(pgorb_ctx* c, int mode, pgorb_track_state* state, const pgorb_trajectory_record* last_record, int nkf,
        const pgorb_kf_pose* kf_pose, pgorb_kf_pose* pose_out)
{
    if (!c) return PGORB_E_ARG;
    if ((mode != PGORB_TRACK_MOTION_MODEL && mode != PGORB_TRACK_REFERENCE_KF) || !state || !pose_out || nkf < 0 || (nkf && !kf_pose))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_track_predict: an unknown mode, a negative count, or an array that is read or written is NULL");
    if (nkf > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_track_predict: more than PGORB_COVIS_MAX_KF key frames");
    const size_t K = (size_t)std::max(nkf, 1), pb = sizeof(pgorb_kf_pose);
    PgHostCall s(c);
    const size_t oRec = s.region(PG_UP, sizeof(*last_record)), oCnt = s.region(PG_UP, 4), oKf = s.region(PG_UP, K * pb),
                 oSt = s.region(PG_INOUT, sizeof(*state)), oOut = s.region(PG_DOWN, pb), oStat = s.region(PG_DOWN, 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oRec, last_record, sizeof(*last_record), 0, sizeof(*last_record));
    *s.host<int32_t>(oCnt) = last_record ? 1 : 0;
    s.put(oKf, kf_pose, (size_t)nkf * pb, 0, K * pb);
    s.put(oSt, state, sizeof(*state));
    if ((rc = s.run([&] {
            return pgorb_track_predict_batch_device(c, 1, mode, nullptr, s.dev<pgorb_track_state>(oSt), s.dev<pgorb_trajectory_record>(oRec), 1,
                s.dev<int32_t>(oCnt), nkf, s.dev<pgorb_kf_pose>(oKf), s.dev<pgorb_kf_pose>(oOut), s.dev<int32_t>(oStat), nullptr); }))) return rc;
    memcpy(state, s.host(oSt), sizeof(*state));
    memcpy(pose_out, s.host(oOut), pb);
    return *s.host<int32_t>(oStat);
}

int pgorb_track_commit(pgorb_ctx* c, pgorb_track_state* state, const pgorb_kf_pose* pose, int ok, int ref_kf, double frame_time,
        int64_t frame_id, int nkf, const pgorb_kf_pose* kf_pose, pgorb_trajectory_record* traj, int traj_cap, int32_t* ntrajectory)
{
    if (!c) return PGORB_E_ARG;
    if (!state || !pose || !ntrajectory || nkf < 0 || traj_cap < 0 || *ntrajectory < 0 || (nkf && !kf_pose) || (traj_cap && !traj))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_track_commit: a negative count, or an array that is read or written is NULL");
    if (nkf > PGORB_COVIS_MAX_KF || traj_cap > PGORB_TRAJ_MAX_RECORDS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_track_commit: more than PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
    // only the record at the count can be written: the device call sees a one-record array that is full exactly when the caller's is
    const int cnt = *ntrajectory;
    const bool room = cnt >= 0 && cnt < traj_cap;
    const size_t K = (size_t)std::max(nkf, 1), pb = sizeof(pgorb_kf_pose), rb = sizeof(pgorb_trajectory_record);
    PgHostCall s(c);
    const size_t oPose = s.region(PG_UP, pb), oOk = s.region(PG_UP, 1), oRef = s.region(PG_UP, 4), oTime = s.region(PG_UP, 8), oId = s.region(PG_UP, 8),
                 oKf = s.region(PG_UP, K * pb), oSt = s.region(PG_INOUT, sizeof(*state)), oRec = s.region(PG_INOUT, rb), oCnt = s.region(PG_INOUT, 4),
                 oStat = s.region(PG_DOWN, 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oPose, pose, pb);
    *s.host<uint8_t>(oOk) = ok ? 1 : 0; *s.host<int32_t>(oRef) = ref_kf; *s.host<double>(oTime) = frame_time; *s.host<int64_t>(oId) = frame_id;
    s.put(oKf, kf_pose, (size_t)nkf * pb, 0, K * pb);
    s.put(oSt, state, sizeof(*state));
    s.put(oRec, room ? traj + cnt : nullptr, rb, 0, rb);
    *s.host<int32_t>(oCnt) = room ? 0 : 1;
    if ((rc = s.run([&] {
            return pgorb_track_commit_batch_device(c, 1, s.dev<pgorb_track_state>(oSt), s.dev<pgorb_kf_pose>(oPose), s.dev(oOk), s.dev<int32_t>(oRef),
                s.dev<double>(oTime), s.dev<int64_t>(oId), nkf, s.dev<pgorb_kf_pose>(oKf), s.dev<pgorb_trajectory_record>(oRec), 1,
                s.dev<int32_t>(oCnt), s.dev<int32_t>(oStat), nullptr); }))) return rc;
    const int status = *s.host<int32_t>(oStat);
    if (!status) {
        memcpy(state, s.host(oSt), sizeof(*state));
        memcpy(traj + cnt, s.host(oRec), rb);
        *ntrajectory = cnt + 1;
    }
    return status;
}

int pgorb_keyframe_tcp(pgorb_ctx* c, int nkf, const pgorb_kf_pose* pose, const int32_t* parent, int nrecord, const int32_t* record,
        float* tcp, int32_t* info_out)
{
    if (!c) return PGORB_E_ARG;
    if (nkf < 0 || nrecord < 0 || !info_out || (nrecord && !record) || (nkf && (!pose || !parent || !tcp)))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_tcp: a negative count, or an array that is read or written is NULL");
    if (nkf > PGORB_COVIS_MAX_KF || nrecord > PGORB_COVIS_MAX_KF)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_keyframe_tcp: more than PGORB_COVIS_MAX_KF key frames or records");
    const size_t K = (size_t)std::max(nkf, 1), NR = (size_t)std::max(nrecord, 1), pb = sizeof(pgorb_kf_pose);
    PgHostCall s(c);
    const size_t oPose = s.region(PG_UP, K * pb), oPar = s.region(PG_UP, K * 4), oRec = s.region(PG_UP, NR * 16), oCi = s.region(PG_UP, 16),
                 oTcp = s.region(PG_INOUT, K * 48), oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oPose, pose, (size_t)nkf * pb, 0, K * pb); s.put(oPar, parent, (size_t)nkf * 4, 0, K * 4);
    s.put(oRec, record, (size_t)nrecord * 16, 0, NR * 16);
    const int32_t ci[4] = {0, nrecord, 0, 0};
    s.put(oCi, ci, 16);
    s.put(oTcp, tcp, (size_t)nkf * 48, 0, K * 48);
    if ((rc = s.run([&] {
            return pgorb_keyframe_tcp_device(c, nkf, s.dev<pgorb_kf_pose>(oPose), s.dev<int32_t>(oPar), nrecord, s.dev<int32_t>(oRec),
                s.dev<int32_t>(oCi), s.dev<float>(oTcp), s.dev<int32_t>(oInfo), nullptr); }))) return rc;
    if (nkf) memcpy(tcp, s.host(oTcp), (size_t)nkf * 48);
    memcpy(info_out, s.host(oInfo), PGORB_TCP_INFO * 4);
    return info_out[1];
}

int pgorb_get_trajectory(pgorb_ctx* c, int nkf, const pgorb_kf_pose* pose, const uint8_t* kf_bad, const int32_t* parent, const uint64_t* kf_id,
        const float* tcp, int n, const pgorb_trajectory_record* traj, double* quat_wxyz, double* translation, int64_t* time_usec,
        int64_t* frame_id, uint8_t* is_lost, int32_t* status, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const std::string fn = "pgorb_get_trajectory: ";
    const char* why = nullptr;
    if (nkf < 0 || n < 0) why = "a count is negative";
    else if (!info || (nkf && (!pose || !kf_bad || !parent || !kf_id || !tcp)) ||
             (n && (!traj || !quat_wxyz || !translation || !time_usec || !frame_id || !is_lost || !status)))
        why = "an array that is read or written is NULL";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    if (nkf > PGORB_COVIS_MAX_KF || n > PGORB_TRAJ_MAX_RECORDS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_get_trajectory: more than PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
    bool live = false;
    for (int k = 0; !why && k < nkf; k++) {
        if (!kf_bad[k]) live = true;
        else if (parent[k] < 0 || parent[k] >= nkf) why = "a bad key frame has no parent or one out of range";
    }
    if (!why && !live) why = "no live key frame";
    for (int i = 0; !why && i < n; i++) {
        const double us = traj[i].frame_time * 1e6;
        if (!std::isfinite(traj[i].frame_time) || !(us >= -9223372036854775808.0 && us < 9223372036854775808.0)) why = "a frame time is not finite or outside int64 microseconds";
        else if (!traj[i].lost && (traj[i].ref_kf < 0 || traj[i].ref_kf >= nkf)) why = "a record's reference key frame is out of range";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    const size_t K = (size_t)nkf, N = (size_t)std::max(n, 1), pb = sizeof(pgorb_kf_pose), rb = sizeof(pgorb_trajectory_record);
    PgHostCall s(c);
    const size_t oPose = s.region(PG_UP, K * pb), oBad = s.region(PG_UP, K), oPar = s.region(PG_UP, K * 4), oId = s.region(PG_UP, K * 8),
                 oTcp = s.region(PG_UP, K * 48), oTraj = s.region(PG_UP, N * rb), oQ = s.region(PG_DOWN, N * 32), oT = s.region(PG_DOWN, N * 24),
                 oTu = s.region(PG_DOWN, N * 8), oFi = s.region(PG_DOWN, N * 8), oLost = s.region(PG_DOWN, N), oStat = s.region(PG_DOWN, N * 4),
                 oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oPose, pose, K * pb); s.put(oBad, kf_bad, K); s.put(oPar, parent, K * 4); s.put(oId, kf_id, K * 8); s.put(oTcp, tcp, K * 48);
    s.put(oTraj, traj, (size_t)n * rb, 0, N * rb);
    if ((rc = s.run([&] {
            return pgorb_get_trajectory_device(c, nkf, s.dev<pgorb_kf_pose>(oPose), s.dev(oBad), s.dev<int32_t>(oPar), s.dev<uint64_t>(oId),
                s.dev<float>(oTcp), n, s.dev<pgorb_trajectory_record>(oTraj), nullptr, s.dev<double>(oQ), s.dev<double>(oT), s.dev<int64_t>(oTu),
                s.dev<int64_t>(oFi), s.dev(oLost), s.dev<int32_t>(oStat), s.dev<int32_t>(oInfo), nullptr); }))) return rc;
    int good = 0;
    if (n) {
        memcpy(quat_wxyz, s.host(oQ), (size_t)n * 32); memcpy(translation, s.host(oT), (size_t)n * 24);
        memcpy(time_usec, s.host(oTu), (size_t)n * 8); memcpy(frame_id, s.host(oFi), (size_t)n * 8);
        memcpy(is_lost, s.host(oLost), (size_t)n); memcpy(status, s.host(oStat), (size_t)n * 4);
        for (int i = 0; i < n; i++) good += !is_lost[i] && !(status[i] & PGORB_TRAJ_BROKEN);
    }
    memcpy(info, s.host(oInfo), PGORB_TRAJ_INFO * 4);
    return good;
}

}  // extern "C"
