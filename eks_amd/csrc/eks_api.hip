// extern "C" entry points of libeks_hip.so (declared in include/eks_hip.h): argument checks and
// dispatch between the scalar-chain path (EKS_FLAG_DIAG_MODEL) and the general small-matrix path.
#include <hip/hip_runtime.h>

#include "eks_adam.hpp"
#include "eks_diag_lane.hpp"
#include <chrono>

#include "eks_internal.hpp"

using namespace eks;

static int check_dims(const eks_dims_t* d) {
  if (!d) return EKS_ERR_NULL;
  if (d->n_keypoints <= 0 || d->n_frames <= 0 || d->state_dim <= 0 || d->obs_dim <= 0)
    return EKS_ERR_SHAPE;
  if ((d->flags & EKS_FLAG_DIAG_MODEL) && d->state_dim != d->obs_dim) return EKS_ERR_SHAPE;
  if ((d->flags & EKS_FLAG_UNIT_AC) && !(d->flags & EKS_FLAG_DIAG_MODEL)) return EKS_ERR_UNSUPPORTED;
  if ((long)d->n_keypoints * d->state_dim > (1L << 24)) return EKS_ERR_SHAPE;
  return EKS_OK;
}

// The model-taking entries (eks_smooth, _tv, _robust, _robust_group, _jumps, _heavy, _heavy_fit, _increments, eks_em_stats, eks_innovations, eks_sample,
// eks_nll, eks_nll_argmin) share one tail, stated once here.  Each entry keeps its own shape check in front of it; the
// ORDER of an entry's checks is part of its contract (tests/test_api_refusals_cpu.py pins every status).

// the caller's eight model pointers; r is var, or rconst on the NLL entries (where s is the candidates)
struct ModelArgs {
  const float* y;
  const void* r;
  const double *m0, *S0, *A, *C, *Q, *s;
};

// EKS_ERR_WORKSPACE for no workspace or one below `need` (0: the size is diag_X / dense_X's own to test)
static int workspace_status(const void* workspace, size_t workspace_bytes, size_t need = 0) {
  return !workspace || workspace_bytes < need ? EKS_ERR_WORKSPACE : EKS_OK;
}

// The eight-pointer null test, then `rest` - the status of the entry's LATER checks (its other pointers, the workspace,
// the size), which are host arithmetic and so may be evaluated by the caller up front - then the dispatch: scalar
// chains (EKS_FLAG_DIAG_MODEL) get a DiagModel in `diag`, general models a DenseModel in `dense`.  d has been checked.
template <class Diag, class Dense>
static int model_call(const eks_dims_t* d, const ModelArgs& a, int rest, Diag diag, Dense dense) {
  if (!a.y || !a.r || !a.m0 || !a.S0 || !a.A || !a.C || !a.Q || !a.s) return EKS_ERR_NULL;
  if (rest != EKS_OK) return rest;
  if (d->flags & EKS_FLAG_DIAG_MODEL) return diag(DiagModel{a.m0, a.S0, a.A, a.C, a.Q, a.s, d->state_dim});
  return dense(DenseModel{a.m0, a.S0, a.A, a.C, a.Q, a.s});
}

// A workspace query: 0 where the entry's shape check (`status`) refuses, else diag(T, N) or dense(T, K, D, O).
template <class Diag, class Dense>
static size_t model_bytes(const eks_dims_t* d, int status, Diag diag, Dense dense) {
  if (status != EKS_OK) return 0;
  if (d->flags & EKS_FLAG_DIAG_MODEL) return diag(d->n_frames, d->n_keypoints * d->state_dim);
  return dense(d->n_frames, d->n_keypoints, d->state_dim, d->obs_dim);
}

// shapes eks_smooth_tv takes (EKS_OK) or the status it refuses them with; nothing here touches the device
static int smooth_tv_check(const eks_dims_t* d) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (d->flags & EKS_FLAG_DIAG_MODEL) return diag_smooth_tv_check(*d);
  if (d->state_dim > 6 || d->obs_dim > 64) return EKS_ERR_UNSUPPORTED;
  return dense_smooth_tv_workspace_bytes(d->n_frames, d->n_keypoints, d->state_dim, d->obs_dim) ? EKS_OK : EKS_ERR_SHAPE;
}

// eks_smooth_robust, eks_smooth_robust_group and eks_smooth_jumps: one entry around two pairs of kernels whose signatures agree; `plane` is the
// weights of the one and the scales of the other, `need` the entry's workspace query.  Order: eks_smooth_tv's shapes and
// refusals, nu / n_iters, the model's pointers, the outputs and a plane that is to be read, the workspace, its size.
template <class Need, class Diag, class Dense>
static int smooth_iterated(const eks_dims_t* d, const ModelArgs& a, double nu, int32_t n_iters, float* plane,
                           int32_t plane_in, float* change, float* ms, float* Vs, void* workspace, size_t workspace_bytes,
                           eks_stream_t stream, Need need, Diag diag, Dense dense) {
  const int rc = smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (!(nu > 0.0) || !(nu <= 1.7e308) || n_iters < 1) return EKS_ERR_SHAPE;
  auto run = [&](auto kernels, const auto& M) {
    return kernels(*d, a.y, static_cast<const float*>(a.r), M, nu, n_iters, plane, plane_in, change, ms, Vs, workspace,
                   workspace_bytes, reinterpret_cast<hipStream_t>(stream));
  };
  return model_call(
      d, a, !ms || !Vs || (plane_in && !plane) ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes, need(d)),
      [&](const DiagModel& M) { return run(diag, M); }, [&](const DenseModel& M) { return run(dense, M); });
}

extern "C" {

const char* eks_version(void) { return "eks_hip 0.1 (gfx950)"; }

const char* eks_status_string(int status) {
  switch (status) {
    case EKS_OK: return "ok";
    case EKS_ERR_NULL: return "null pointer";
    case EKS_ERR_SHAPE: return "bad shape";
    case EKS_ERR_UNSUPPORTED: return "unsupported (D, O) / flag combination";
    case EKS_ERR_WORKSPACE: return "workspace missing or too small";
    case EKS_CSV_IO: return "file cannot be opened or mapped";
    case EKS_CSV_FALLBACK: return "not a purely numeric table: read it with pandas";
    default: return status <= EKS_ERR_HIP_BASE ? hipGetErrorString((hipError_t)(EKS_ERR_HIP_BASE - status))
                                               : "unknown status";
  }
}

size_t eks_smooth_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, check_dims(d), diag_smooth_workspace_bytes, dense_smooth_workspace_bytes);
}

int eks_smooth(const eks_dims_t* d, const float* y, const float* var, const double* m0,
               const double* S0, const double* A, const double* C, const double* Q,
               const double* s, float* ms, float* Vs, void* workspace, size_t workspace_bytes,
               eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s}, !ms || !Vs ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](const DiagModel& M) { return diag_smooth(*d, y, var, M, ms, Vs, workspace, workspace_bytes, st); },
      [&](const DenseModel& M) { return dense_smooth(*d, y, var, M, ms, Vs, workspace, workspace_bytes, st); });
}

size_t eks_smooth_tv_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, smooth_tv_check(d), diag_em_workspace_bytes, dense_smooth_tv_workspace_bytes);
}

int eks_smooth_tv(const eks_dims_t* d, const float* y, const float* var, const float* qscale,
                  int32_t qscale_per_keypoint, const double* m0, const double* S0, const double* A, const double* C,
                  const double* Q, const double* s, float* ms, float* Vs, void* workspace, size_t workspace_bytes,
                  eks_stream_t stream) {
  const int rc = smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s},
      !qscale || !ms || !Vs ? EKS_ERR_NULL
                            : workspace_status(workspace, workspace_bytes, eks_smooth_tv_workspace_bytes(d)),
      [&](const DiagModel& M) {
        return diag_smooth_tv(*d, y, var, qscale, qscale_per_keypoint, M, ms, Vs, workspace, workspace_bytes, st);
      },
      [&](const DenseModel& M) {
        return dense_smooth_tv(*d, y, var, qscale, qscale_per_keypoint, M, ms, Vs, workspace, workspace_bytes, st);
      });
}

size_t eks_smooth_robust_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, smooth_tv_check(d), diag_smooth_robust_workspace_bytes, dense_smooth_robust_workspace_bytes);
}

size_t eks_smooth_jumps_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(
      d, smooth_tv_check(d), [d](int T, int) { return diag_smooth_jumps_workspace_bytes(T, d->n_keypoints, d->state_dim); },
      dense_smooth_jumps_workspace_bytes);
}

int eks_smooth_robust(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                      const double* A, const double* C, const double* Q, const double* s, double nu, int32_t n_iters,
                      float* weights, int32_t weights_in, float* change, float* ms, float* Vs, void* workspace,
                      size_t workspace_bytes, eks_stream_t stream) {
  return smooth_iterated(d, {y, var, m0, S0, A, C, Q, s}, nu, n_iters, weights, weights_in, change, ms, Vs, workspace,
                         workspace_bytes, stream, eks_smooth_robust_workspace_bytes, diag_smooth_robust,
                         dense_smooth_robust);
}

int eks_smooth_jumps(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, const double* s, double nu, int32_t n_iters,
                     float* scales, int32_t scales_in, float* change, float* ms, float* Vs, void* workspace,
                     size_t workspace_bytes, eks_stream_t stream) {
  return smooth_iterated(d, {y, var, m0, S0, A, C, Q, s}, nu, n_iters, scales, scales_in, change, ms, Vs, workspace,
                         workspace_bytes, stream, eks_smooth_jumps_workspace_bytes, diag_smooth_jumps,
                         dense_smooth_jumps);
}

// eks_smooth_robust's shapes, then the group: at least 1 and a divisor of O
static int robust_group_check(const eks_dims_t* d, int32_t group) {
  const int rc = smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  return group < 1 || d->obs_dim % group != 0 ? EKS_ERR_SHAPE : EKS_OK;
}

size_t eks_smooth_robust_group_workspace_bytes(const eks_dims_t* d, int32_t group) {
  if (robust_group_check(d, group) == EKS_OK && group == 1) return eks_smooth_robust_workspace_bytes(d);
  return model_bytes(
      d, robust_group_check(d, group), [group](int T, int N) { return diag_smooth_robust_group_workspace_bytes(T, N, group); },
      [group](int T, int K, int D, int O) { return dense_smooth_robust_group_workspace_bytes(T, K, D, O, group); });
}

// eks_smooth_robust's order with the group's check behind the shapes; group = 1 IS eks_smooth_robust
int eks_smooth_robust_group(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                            const double* A, const double* C, const double* Q, const double* s, double nu, int32_t group,
                            int32_t n_iters, float* weights, int32_t weights_in, float* change, float* ms, float* Vs,
                            void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = robust_group_check(d, group);
  if (rc != EKS_OK) return rc;
  if (group == 1)
    return eks_smooth_robust(d, y, var, m0, S0, A, C, Q, s, nu, n_iters, weights, weights_in, change, ms, Vs, workspace,
                             workspace_bytes, stream);
  return smooth_iterated(
      d, {y, var, m0, S0, A, C, Q, s}, nu, n_iters, weights, weights_in, change, ms, Vs, workspace, workspace_bytes,
      stream, [group](const eks_dims_t* dd) { return eks_smooth_robust_group_workspace_bytes(dd, group); },
      [group](const eks_dims_t& dd, const float* yy, const float* vv, const DiagModel& M, double nu_, int n, float* w,
              int w_in, float* ch, float* ms_, float* Vs_, void* ws, size_t wsb, hipStream_t st) {
        return diag_smooth_robust_group(dd, yy, vv, M, nu_, group, n, w, w_in, ch, ms_, Vs_, ws, wsb, st);
      },
      [group](const eks_dims_t& dd, const float* yy, const float* vv, const DenseModel& M, double nu_, int n, float* w,
              int w_in, float* ch, float* ms_, float* Vs_, void* ws, size_t wsb, hipStream_t st) {
        return dense_smooth_robust_group(dd, yy, vv, M, nu_, group, n, w, w_in, ch, ms_, Vs_, ws, wsb, st);
      });
}

size_t eks_smooth_heavy_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(
      d, smooth_tv_check(d), [d](int T, int) { return diag_smooth_heavy_workspace_bytes(T, d->n_keypoints, d->state_dim); },
      dense_smooth_heavy_workspace_bytes);
}

// eks_smooth_jumps' order with two nu and two planes: shapes, either nu / n_iters, the model's pointers, the outputs
// and a plane that is to be read, the workspace, its size
int eks_smooth_heavy(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, const double* s, double nu_obs, double nu_proc,
                     int32_t n_iters, float* weights, float* scales, int32_t planes_in, float* change, float* ms,
                     float* Vs, void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  if (!(nu_obs > 0.0) || !(nu_obs <= 1.7e308) || !(nu_proc > 0.0) || !(nu_proc <= 1.7e308) || n_iters < 1)
    return EKS_ERR_SHAPE;
  const bool plane_missing = ((planes_in & 1) && !weights) || ((planes_in & 2) && !scales);
  auto run = [&](auto kernels, const auto& M) {
    return kernels(*d, y, var, M, nu_obs, nu_proc, n_iters, weights, scales, planes_in, change, ms, Vs, workspace,
                   workspace_bytes, reinterpret_cast<hipStream_t>(stream));
  };
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s},
      !ms || !Vs || plane_missing ? EKS_ERR_NULL
                                  : workspace_status(workspace, workspace_bytes, eks_smooth_heavy_workspace_bytes(d)),
      [&](const DiagModel& M) { return run(diag_smooth_heavy, M); },
      [&](const DenseModel& M) { return run(dense_smooth_heavy, M); });
}

// shapes eks_smooth_heavy_fit takes: eks_smooth_heavy's with T >= 2 (n = D (T - 1) divides)
static int heavy_fit_check(const eks_dims_t* d) {
  const int rc = smooth_tv_check(d);
  if (rc != EKS_OK) return rc;
  return d->n_frames < 2 ? EKS_ERR_SHAPE : EKS_OK;
}

size_t eks_smooth_heavy_fit_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(
      d, heavy_fit_check(d),
      [d](int T, int) { return diag_smooth_heavy_fit_workspace_bytes(T, d->n_keypoints, d->state_dim); },
      dense_smooth_heavy_fit_workspace_bytes);
}

// eks_smooth_heavy's order with the fit's own refusals behind the shapes: shapes and T >= 2; either nu (+inf allowed),
// the bounds, n_iters and an input plane on a Gaussian side (EKS_ERR_SHAPE); nu_obs = +inf on a general model
// (EKS_ERR_UNSUPPORTED); the model's pointers; s_out, the outputs and a plane that is to be read; the workspace, its
// size.  Only then is anything enqueued: the copy of s into s_out first.
int eks_smooth_heavy_fit(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                         const double* A, const double* C, const double* Q, const double* s, double nu_obs,
                         double nu_proc, int32_t n_iters, double log_s_lo, double log_s_hi, float* weights,
                         float* scales, int32_t planes_in, float* change, double* s_out, float* ms, float* Vs,
                         void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = heavy_fit_check(d);
  if (rc != EKS_OK) return rc;
  const bool obs_gauss = nu_obs > 1.7e308, proc_gauss = nu_proc > 1.7e308;
  if (!(nu_obs > 0.0) || !(nu_proc > 0.0) || n_iters < 1) return EKS_ERR_SHAPE;
  if (!(log_s_lo <= log_s_hi) || !(log_s_lo >= -1.7e308) || !(log_s_hi <= 1.7e308)) return EKS_ERR_SHAPE;
  if ((obs_gauss && (planes_in & 1)) || (proc_gauss && (planes_in & 2))) return EKS_ERR_SHAPE;
  if (obs_gauss && !(d->flags & EKS_FLAG_DIAG_MODEL)) return EKS_ERR_UNSUPPORTED;
  const bool plane_missing = ((planes_in & 1) && !weights) || ((planes_in & 2) && !scales);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto run = [&](auto kernels, auto M) {
    if (s_out != s) {
      const hipError_t e = hipMemcpyAsync(s_out, s, (size_t)d->n_keypoints * sizeof(double), hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return EKS_ERR_HIP_BASE - (int)e;
    }
    M.s = s_out;
    return kernels(*d, y, var, M, s_out, nu_obs, nu_proc, n_iters, log_s_lo, log_s_hi, weights, scales, planes_in, change,
                   ms, Vs, workspace, workspace_bytes, st);
  };
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s},
      !s_out || !ms || !Vs || plane_missing
          ? EKS_ERR_NULL
          : workspace_status(workspace, workspace_bytes, eks_smooth_heavy_fit_workspace_bytes(d)),
      [&](const DiagModel& M) { return run(diag_smooth_heavy_fit, M); },
      [&](const DenseModel& M) { return run(dense_smooth_heavy_fit, M); });
}

// shapes eks_smooth_increments takes (EKS_OK) or the status it refuses them with; nothing here touches the device
static int increments_check(const eks_dims_t* d) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (d->flags & EKS_FLAG_DIAG_MODEL) {
    if (!(d->flags & EKS_FLAG_VS_DIAG)) return EKS_ERR_UNSUPPORTED;   // off-diagonals are identically zero
    return diag_chain_covers(d->n_frames, d->n_keypoints * d->state_dim) ? EKS_OK : EKS_ERR_SHAPE;
  }
  if (d->state_dim > 6 || d->obs_dim > 64) return EKS_ERR_UNSUPPORTED;
  return EKS_OK;
}

size_t eks_smooth_increments_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, increments_check(d), diag_increments_workspace_bytes, dense_increments_workspace_bytes);
}

int eks_smooth_increments(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                          const double* A, const double* C, const double* Q, const double* s, float* ms, float* Vs,
                          float* lag1, float* dmean, float* dV, void* workspace, size_t workspace_bytes,
                          eks_stream_t stream) {
  const int rc = increments_check(d);
  if (rc != EKS_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s},
      !lag1 && !dmean && !dV ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](const DiagModel& M) {
        return diag_increments(*d, y, var, M, ms, Vs, lag1, dmean, dV, workspace, workspace_bytes, st);
      },
      [&](const DenseModel& M) {
        return dense_increments(*d, y, var, M, ms, Vs, lag1, dmean, dV, workspace, workspace_bytes, st);
      });
}

// shapes eks_em_stats takes (EKS_OK) or the status it refuses them with; nothing here touches the device
static int em_check(const eks_dims_t* d) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (d->flags & EKS_FLAG_DIAG_MODEL) {
    if (!(d->flags & EKS_FLAG_VS_DIAG)) return EKS_ERR_UNSUPPORTED;   // a diagonal Q's M-step reads the diagonal only
    return diag_chain_covers(d->n_frames, d->n_keypoints * d->state_dim) ? EKS_OK : EKS_ERR_SHAPE;
  }
  if (d->state_dim > 6 || d->obs_dim > 64) return EKS_ERR_UNSUPPORTED;
  // (dense_em_stats' own launch-index check, here so that the workspace query and the call agree)
  return dense_em_workspace_bytes(d->n_frames, d->n_keypoints, d->state_dim, d->obs_dim) ? EKS_OK : EKS_ERR_SHAPE;
}

size_t eks_em_stats_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, em_check(d), diag_em_workspace_bytes, dense_em_workspace_bytes);
}

int eks_em_stats(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                 const double* A, const double* C, const double* Q, const double* s, double* Sw, void* workspace,
                 size_t workspace_bytes, eks_stream_t stream) {
  const int rc = em_check(d);
  if (rc != EKS_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s},
      !Sw ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes, eks_em_stats_workspace_bytes(d)),
      [&](const DiagModel& M) { return diag_em_stats(*d, y, var, M, Sw, workspace, workspace_bytes, st); },
      [&](const DenseModel& M) { return dense_em_stats(*d, y, var, M, Sw, workspace, workspace_bytes, st); });
}

// shapes eks_innovations takes (EKS_OK) or the status it refuses them with; nothing here touches the device.
// EKS_FLAG_VS_DIAG is ignored: no output is a covariance matrix
static int innovations_check(const eks_dims_t* d) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (d->flags & EKS_FLAG_DIAG_MODEL)
    return diag_chain_covers(d->n_frames, d->n_keypoints * d->state_dim) ? EKS_OK : EKS_ERR_SHAPE;
  if (d->state_dim > 6 || d->obs_dim > 64) return EKS_ERR_UNSUPPORTED;
  return dense_innovations_workspace_bytes(d->n_frames, d->n_keypoints, d->state_dim, d->obs_dim) ? EKS_OK
                                                                                                    : EKS_ERR_SHAPE;
}

size_t eks_innovations_workspace_bytes(const eks_dims_t* d) {
  return model_bytes(d, innovations_check(d), diag_em_workspace_bytes, dense_innovations_workspace_bytes);
}

int eks_innovations(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                    const double* A, const double* C, const double* Q, const double* s, float* innov,
                    float* innov_var, float* nis, float* frame_ll, double* loglik, void* workspace,
                    size_t workspace_bytes, eks_stream_t stream) {
  const int rc = innovations_check(d);
  if (rc != EKS_OK) return rc;
  int rest = workspace_status(workspace, workspace_bytes, eks_innovations_workspace_bytes(d));
  if (!innov && !innov_var && !nis && !frame_ll && !loglik) rest = EKS_ERR_NULL;
  // scalar chains: nis and frame_ll are elementwise functions of innov and innov_var
  else if ((d->flags & EKS_FLAG_DIAG_MODEL) && (nis || frame_ll)) rest = EKS_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s}, rest,
      [&](const DiagModel& M) {
        return diag_innovations(*d, y, var, M, innov, innov_var, loglik, workspace, workspace_bytes, st);
      },
      [&](const DenseModel& M) {
        return dense_innovations(*d, y, var, M, innov, innov_var, nis, frame_ll, loglik, workspace, workspace_bytes, st);
      });
}

// shapes the M-step for the scale takes: eks_em_stats' with T >= 2 (n = D (T - 1) divides) and, on general models,
// the full D x D statistic (tr(Q^-1 Sw) needs its off-diagonals)
static int em_scale_check(const eks_dims_t* d, int32_t n_blocks, int32_t max_iters) {
  const int rc = em_check(d);
  if (rc != EKS_OK) return rc;
  if (d->n_frames < 2 || n_blocks <= 0 || max_iters < 0) return EKS_ERR_SHAPE;
  if (!(d->flags & EKS_FLAG_DIAG_MODEL) && (d->flags & EKS_FLAG_VS_DIAG)) return EKS_ERR_UNSUPPORTED;
  return EKS_OK;
}

int eks_em_scale_step(const eks_dims_t* d, const double* Q, const double* Sw, int32_t n_blocks,
                      const int32_t* block_offsets, const int32_t* block_members, double lo, double hi, double tol,
                      int32_t max_iters, double* state, double* s_keypoint, int32_t* n_active, eks_stream_t stream) {
  const int rc = em_scale_check(d, n_blocks, max_iters);
  if (rc != EKS_OK) return rc;
  if (!Q || !Sw || !block_offsets || !block_members || !state || !s_keypoint || !n_active) return EKS_ERR_NULL;
  return em_scale_step(*d, Q, Sw, n_blocks, block_offsets, block_members, lo, hi, tol, max_iters, state, s_keypoint,
                       n_active, reinterpret_cast<hipStream_t>(stream));
}

int eks_em_scale_run(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, int32_t n_blocks,
                     const int32_t* block_offsets, const int32_t* block_members, double lo, double hi, double tol,
                     int32_t max_iters, int32_t n_iters, double* state, double* s_keypoint, double* Sw,
                     int32_t* n_active, void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  if (n_iters < 0) return EKS_ERR_SHAPE;
  const int rc = em_scale_check(d, n_blocks, max_iters);
  if (rc != EKS_OK) return rc;
  if (!(d->flags & EKS_FLAG_DIAG_MODEL) && !(d->flags & EKS_FLAG_Q_PD)) return EKS_ERR_UNSUPPORTED;   // Q^-1
  if (!y || !var || !m0 || !S0 || !A || !C || !Q || !block_offsets || !block_members || !state || !s_keypoint || !Sw ||
      !n_active)
    return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  if (workspace_bytes < eks_em_stats_workspace_bytes(d)) return EKS_ERR_WORKSPACE;
  for (int it = 0; it < n_iters; ++it) {   // back to back on the stream, no host round trip
    int rc2 = eks_em_stats(d, y, var, m0, S0, A, C, Q, s_keypoint, Sw, workspace, workspace_bytes, stream);
    if (rc2 != EKS_OK) return rc2;
    rc2 = eks_em_scale_step(d, Q, Sw, n_blocks, block_offsets, block_members, lo, hi, tol, max_iters, state, s_keypoint,
                            n_active, stream);
    if (rc2 != EKS_OK) return rc2;
  }
  return EKS_OK;
}

int32_t eks_sample_noise_width(const eks_dims_t* d) {
  if (check_dims(d) != EKS_OK) return 0;
  return (d->flags & EKS_FLAG_DIAG_MODEL) ? d->state_dim : d->state_dim + d->obs_dim;
}

size_t eks_sample_workspace_bytes(const eks_dims_t* d, int32_t n_draws) {
  return model_bytes(
      d, n_draws < 1 ? EKS_ERR_SHAPE : check_dims(d),
      [&](int T, int N) { return diag_sample_workspace_bytes(T, N, n_draws); },
      [&](int T, int K, int D, int O) -> size_t {
        if (D > 6 || O > 64) return 0;
        if (((size_t)n_draws + 1) * K * D > (1u << 24)) return 0;   // eks_sample: EKS_ERR_SHAPE
        return dense_sample_workspace_bytes(T, K, D, O, n_draws);
      });
}

int eks_sample(const eks_dims_t* d, const float* y, const float* var, const double* m0, const double* S0,
               const double* A, const double* C, const double* Q, const double* s, int32_t n_draws, uint64_t seed,
               int32_t first_keypoint, int32_t first_draw, const float* noise, float* ms, float* draws,
               void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_draws < 1 || first_keypoint < 0 || first_draw < 0) return EKS_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s}, !draws ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](const DiagModel& M) {
        return diag_sample(*d, y, var, M, n_draws, seed, first_keypoint, first_draw, noise, ms, draws, workspace,
                           workspace_bytes, st);
      },
      [&](const DenseModel& M) {
        return dense_sample(*d, y, var, M, n_draws, seed, first_keypoint, first_draw, noise, ms, draws, workspace,
                            workspace_bytes, st);
      });
}

// 0 for every shape eks_sample_tv refuses
size_t eks_sample_tv_workspace_bytes(const eks_dims_t* d, int32_t n_draws) {
  return model_bytes(
      d, n_draws < 1 ? EKS_ERR_SHAPE : smooth_tv_check(d),
      [&](int T, int N) { return diag_sample_tv_check(T, N, n_draws) == EKS_OK ? diag_sample_workspace_bytes(T, N, n_draws) : 0; },
      [&](int T, int K, int D, int O) { return dense_sample_tv_workspace_bytes(T, K, D, O, n_draws); });
}

// Order: eks_sample's refusals in eks_sample's order (dims, n_draws / first_*, the model's pointers, draws, the
// workspace, and per path its size and launch-index limits), then eks_smooth_tv's shapes.  Only then is anything enqueued.
int eks_sample_tv(const eks_dims_t* d, const float* y, const float* var, const float* qscale,
                  int32_t qscale_per_keypoint, const float* weights, const double* m0, const double* S0,
                  const double* A, const double* C, const double* Q, const double* s, int32_t n_draws, uint64_t seed,
                  int32_t first_keypoint, int32_t first_draw, const float* noise, float* ms, float* draws,
                  void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_draws < 1 || first_keypoint < 0 || first_draw < 0) return EKS_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, var, m0, S0, A, C, Q, s}, !draws ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](const DiagModel& M) {
        const int T = d->n_frames, N = d->n_keypoints * d->state_dim;
        if (workspace_bytes < diag_sample_workspace_bytes(T, N, n_draws)) return (int)EKS_ERR_WORKSPACE;
        const int r1 = diag_sample_tv_check(T, N, n_draws);
        if (r1 != EKS_OK) return r1;
        const int r2 = diag_smooth_tv_check(*d);
        if (r2 != EKS_OK) return r2;
        return diag_sample_tv(*d, y, var, qscale, qscale_per_keypoint, weights, M, n_draws, seed, first_keypoint,
                              first_draw, noise, ms, draws, workspace, workspace_bytes, st);
      },
      [&](const DenseModel& M) {
        // (dense_sample_tv: eks_sample's limits, which contain eks_smooth_tv's on general models, then the size)
        return dense_sample_tv(*d, y, var, qscale, qscale_per_keypoint, weights, M, n_draws, seed, first_keypoint,
                               first_draw, noise, ms, draws, workspace, workspace_bytes, st);
      });
}

int eks_sample_noise(const eks_dims_t* d, int32_t n_draws, uint64_t seed, int32_t first_keypoint, int32_t first_draw,
                     float* noise, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_draws < 1 || first_keypoint < 0 || first_draw < 0) return EKS_ERR_SHAPE;
  if (!noise) return EKS_ERR_NULL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->flags & EKS_FLAG_DIAG_MODEL)
    return diag_sample_noise(d->n_frames, d->n_keypoints * d->state_dim, d->state_dim, n_draws, seed, first_keypoint,
                             first_draw, noise, st);
  if (d->state_dim + d->obs_dim > 6 + 64) return EKS_ERR_SHAPE;   // wider than any supported model's W = D + O
  if (d->state_dim > 6 || d->obs_dim > 64) return EKS_ERR_UNSUPPORTED;
  return dense_sample_noise(d->n_frames, d->n_keypoints, d->state_dim + d->obs_dim, n_draws, seed, first_keypoint,
                            first_draw, noise, st);
}

size_t eks_const_r_workspace_bytes(const eks_dims_t* d) {
  if (check_dims(d) != EKS_OK) return 0;
  return const_r_workspace_bytes(d->n_frames, d->n_keypoints * d->obs_dim);
}

int eks_const_r(const eks_dims_t* d, const float* var, double min_var, double* rconst,
                void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (!var || !rconst) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  return const_r(d->n_frames, d->n_keypoints * d->obs_dim, var, min_var, rconst, workspace,
                 workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

size_t eks_nll_workspace_bytes(const eks_dims_t* d, int32_t n_cand) {
  return model_bytes(
      d, n_cand <= 0 ? EKS_ERR_SHAPE : check_dims(d), [&](int T, int N) { return diag_nll_workspace_bytes(T, N, n_cand); },
      [&](int T, int K, int D, int O) { return dense_nll_workspace_bytes(T, K, D, O, n_cand); });
}

// (the NLL entries: rconst in the place of var and the candidates in the place of s for the null test; the model the
//  kernels get has no s, as in eks_adam_run)

int eks_nll(const eks_dims_t* d, const float* y, const double* rconst, const double* m0,
            const double* S0, const double* A, const double* C, const double* Q,
            const double* s_cand, int32_t n_cand, int32_t per_keypoint, double* nll, double* dnll,
            void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_cand <= 0) return EKS_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, rconst, m0, S0, A, C, Q, s_cand}, !nll ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](DiagModel M) {
        M.s = nullptr;
        return diag_nll(*d, y, rconst, M, s_cand, n_cand, per_keypoint, nll, dnll, workspace, workspace_bytes, st);
      },
      [&](DenseModel M) {
        M.s = nullptr;
        return dense_nll(*d, y, rconst, M, s_cand, n_cand, per_keypoint, nll, dnll, workspace, workspace_bytes, st);
      });
}

int eks_nll_argmin(const eks_dims_t* d, const float* y, const double* rconst, const double* m0,
                   const double* S0, const double* A, const double* C, const double* Q,
                   const double* s_cand, int32_t n_cand, double* nll, double* s_out, int32_t* idx_out,
                   void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_cand <= 0) return EKS_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return model_call(
      d, {y, rconst, m0, S0, A, C, Q, s_cand},
      !nll || !s_out ? EKS_ERR_NULL : workspace_status(workspace, workspace_bytes),
      [&](DiagModel M) {
        M.s = nullptr;
        return diag_nll(*d, y, rconst, M, s_cand, n_cand, 0, nll, nullptr, workspace, workspace_bytes, st, nullptr, s_out,
                        idx_out);
      },
      [&](DenseModel M) {
        M.s = nullptr;
        const int rc2 = dense_nll(*d, y, rconst, M, s_cand, n_cand, 0, nll, nullptr, workspace, workspace_bytes, st);
        if (rc2 != EKS_OK) return rc2;
        return argmin_s(d->n_keypoints, n_cand, nll, s_cand, s_out, idx_out, st);
      });
}

int eks_order_stats(int32_t n_rows, int32_t n_cols, const float* x, int32_t rank_lo, int32_t rank_hi,
                    float* out, int32_t* nan_count, eks_stream_t stream) {
  if (n_rows <= 0 || n_cols <= 0 || rank_lo < 0 || rank_hi < rank_lo || rank_hi >= n_rows || rank_hi > rank_lo + 1)
    return EKS_ERR_SHAPE;
  if (!x || !out || !nan_count) return EKS_ERR_NULL;
  return order_stats(n_rows, n_cols, x, rank_lo, rank_hi, out, nan_count, reinterpret_cast<hipStream_t>(stream));
}

int eks_np_nanstd_rows(int32_t n_rows, int32_t n_cols, const float* x, const int32_t* leaves, int32_t n_leaves,
                       const int32_t* ops, int32_t n_ops, float* out, eks_stream_t stream) {
  if (n_rows <= 0 || n_cols <= 0 || n_leaves <= 0 || n_ops != n_leaves - 1) return EKS_ERR_SHAPE;
  if (!x || !leaves || !out || (n_ops > 0 && !ops)) return EKS_ERR_NULL;
  return np_nanstd_rows(n_rows, n_cols, x, leaves, n_leaves, ops, n_ops, out, reinterpret_cast<hipStream_t>(stream));
}

int eks_np_nanstd_diff_rows(int32_t n_frames, int32_t n_keypoints, int32_t obs_dim, const float* x, const int32_t* leaves,
                            int32_t n_leaves, const int32_t* ops, int32_t n_ops, float* out, eks_stream_t stream) {
  if (n_frames < 2 || n_keypoints <= 0 || obs_dim <= 0 || n_leaves <= 0 || n_ops != n_leaves - 1) return EKS_ERR_SHAPE;
  if (!x || !leaves || !out || (n_ops > 0 && !ops)) return EKS_ERR_NULL;
  return np_nanstd_diff_rows(n_frames, n_keypoints, obs_dim, x, leaves, n_leaves, ops, n_ops, out,
                             reinterpret_cast<hipStream_t>(stream));
}

int eks_argmin_s(int32_t n_keypoints, int32_t n_cand, const double* nll, const double* s_cand,
                 double* s_out, int32_t* idx_out, eks_stream_t stream) {
  if (n_keypoints <= 0 || n_cand <= 0) return EKS_ERR_SHAPE;
  if (!nll || !s_cand || !s_out) return EKS_ERR_NULL;
  return argmin_s(n_keypoints, n_cand, nll, s_cand, s_out, idx_out,
                  reinterpret_cast<hipStream_t>(stream));
}

int eks_adam_step(int32_t n_blocks, const int32_t* block_offsets, const int32_t* block_members,
                  const double* nll, const double* dnll, double lr, double lo, double hi,
                  double tol, int32_t safety_cap, double* state, double* s_keypoint,
                  int32_t* n_active, eks_stream_t stream) {
  if (n_blocks <= 0) return EKS_ERR_SHAPE;
  if (!block_offsets || !block_members || !nll || !dnll || !state || !s_keypoint || !n_active)
    return EKS_ERR_NULL;
  return adam_step(n_blocks, block_offsets, block_members, nll, dnll, lr, lo, hi, tol, safety_cap,
                   state, s_keypoint, n_active, reinterpret_cast<hipStream_t>(stream));
}

size_t eks_ar1_nll_workspace_bytes(const eks_dims_t* d, int32_t n_tan) {
  if (check_dims(d) != EKS_OK || n_tan < 0) return 0;
  return ar1_nll_workspace_bytes(d->n_frames, d->n_keypoints, d->state_dim, n_tan);
}

int eks_ar1_nll(const eks_dims_t* d, const float* y, const float* var, const double* m0,
                const double* S0, const double* C, const double* a, const double* q,
                const double* da, const double* dq, int32_t n_tan, double* nll, double* dnll,
                void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_tan < 0) return EKS_ERR_SHAPE;
  if (!y || !var || !m0 || !S0 || !C || !a || !q || !nll) return EKS_ERR_NULL;
  if (n_tan > 0 && (!da || !dq || !dnll)) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  return ar1_nll(*d, y, var, m0, S0, C, a, q, da, dq, n_tan, nll, dnll, workspace, workspace_bytes,
                 reinterpret_cast<hipStream_t>(stream));
}

int eks_pupil_adam_step(int32_t n_chains, const double* latent_var, const double* nll,
                        const double* dnll, double lr, double tol, int32_t safety_cap,
                        double* state, double* a, double* q, double* da, double* dq,
                        int32_t* n_active, eks_stream_t stream) {
  if (n_chains <= 0) return EKS_ERR_SHAPE;
  if (!latent_var || !state || !a || !q || !da || !dq || !n_active) return EKS_ERR_NULL;
  if (nll && !dnll) return EKS_ERR_NULL;
  return pupil_adam_step(n_chains, latent_var, nll, dnll, lr, tol, safety_cap, state, a, q, da, dq,
                         n_active, reinterpret_cast<hipStream_t>(stream));
}

int eks_adam_run(const eks_dims_t* d, const float* y, const double* rconst, const double* m0,
                 const double* S0, const double* A, const double* C, const double* Q,
                 int32_t n_blocks, const int32_t* block_offsets, const int32_t* block_members,
                 double lr, double lo, double hi, double tol, int32_t safety_cap, int32_t n_iters,
                 double* state, double* s_keypoint, double* nll, double* dnll, int32_t* n_active,
                 void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  if (n_iters < 0) return EKS_ERR_SHAPE;
  if (!dnll) return EKS_ERR_NULL;
  {
    const int rc0 = check_dims(d);
    if (rc0 != EKS_OK) return rc0;
  }
  if (n_blocks <= 0) return EKS_ERR_SHAPE;
  if (!y || !rconst || !m0 || !S0 || !A || !C || !Q || !block_offsets || !block_members || !state ||
      !s_keypoint || !nll || !n_active)
    return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  if ((d->flags & EKS_FLAG_DIAG_MODEL) && n_iters > 0) {
    // Scalar chains: the loss kernels read the optimiser state and skip the keypoints whose block has
    // stopped (a wave none of whose 64 chains is still running returns at once; results of the others
    // are bit for bit those of the ungated loop), and when every block is one keypoint - the reference's
    // default, blocks = [] (eks/core.py:223-224) - the step is applied by the loss assembly itself:
    // two launches per iteration instead of three.
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int K = d->n_keypoints, N = K * d->state_dim;
    const size_t need = diag_nll_workspace_bytes(d->n_frames, N, 1);
    if (workspace_bytes < need) return EKS_ERR_WORKSPACE;
    char* tail = static_cast<char*>(workspace) + need - adam_extra_bytes(N);
    int32_t* kp_block = reinterpret_cast<int32_t*>(tail);
    int32_t* counter_b = reinterpret_cast<int32_t*>(tail + adam_extra_bytes(N) - 256);
    int rc = adam_prepare(n_blocks, K, block_offsets, block_members, kp_block, n_active, counter_b, st);
    if (rc != EKS_OK) return rc;
    {   // tile tickets of the single-launch loss kernel: zero once, every evaluation leaves them zero
      const hipError_t e = hipMemsetAsync(nll_ws_tickets(workspace, d->n_frames, N, 1), 0,
                                          (size_t)((N + 63) / 64) * sizeof(int32_t), st);
      if (e != hipSuccess) return EKS_ERR_HIP_BASE - (int)e;
    }
    const bool in_kernel = n_blocks == K && diag_nll_grad_tree(d->n_frames, K, d->state_dim);
    const DiagModel M{m0, S0, A, C, Q, nullptr, d->state_dim};
    if (diag_lag_adam_ok(d->n_frames, K, d->state_dim, n_blocks)) {
      // one keypoint per optimiser block, a session long enough for a head and 256 lags: one streaming pass for the lag
      // sums, then all n_iters iterations in ONE launch, a workgroup per keypoint, no pass over y per iteration
      // (eks_lag_adam.hip, round 6); n_active counts the keypoints still running
      const AdamFuse F{block_offsets, block_members, kp_block, lr, lo, hi, tol, safety_cap, 1, state, s_keypoint,
                       n_active, counter_b};
      rc = diag_lag_adam(*d, y, rconst, M, n_iters, nll, dnll, F, workspace, workspace_bytes, st);
      if (rc != EKS_ERR_UNSUPPORTED) return rc;
    }
    if (diag_nll_adam_persist_ok(d->n_frames, K, d->state_dim, n_blocks)) {
      // short sessions, one keypoint per optimiser block: all n_iters iterations in ONE launch, a workgroup per
      // keypoint (eks_diag_nll.hip: diag_nll_adam_persist_kernel); n_active counts the keypoints still running
      const AdamFuse F{block_offsets, block_members, kp_block, lr, lo, hi, tol, safety_cap, 1, state, s_keypoint,
                       n_active, counter_b};
      return diag_nll_adam_persist(*d, y, rconst, M, n_iters, nll, dnll, F, n_active, st);
    }
    for (int it = 0; it < n_iters; ++it) {
      // the LAST iteration of the call counts into n_active, the one before into the spare counter, ...
      const bool last_parity = ((n_iters - 1 - it) & 1) == 0;
      AdamFuse F{block_offsets, block_members, kp_block, lr, lo, hi, tol, safety_cap, in_kernel ? 1 : 0,
                 state, s_keypoint, last_parity ? n_active : counter_b, last_parity ? counter_b : n_active};
      rc = diag_nll(*d, y, rconst, M, s_keypoint, 1, 1, nll, dnll, workspace, workspace_bytes, st, &F);
      if (rc != EKS_OK) return rc;
      if (!in_kernel) {
        rc = adam_step(n_blocks, block_offsets, block_members, nll, dnll, lr, lo, hi, tol, safety_cap, state,
                       s_keypoint, n_active, st);
        if (rc != EKS_OK) return rc;
      }
    }
    return EKS_OK;
  }
  for (int it = 0; it < n_iters; ++it) {
    int rc = eks_nll(d, y, rconst, m0, S0, A, C, Q, s_keypoint, 1, 1, nll, dnll, workspace,
                     workspace_bytes, stream);
    if (rc != EKS_OK) return rc;
    rc = eks_adam_step(n_blocks, block_offsets, block_members, nll, dnll, lr, lo, hi, tol, safety_cap,
                       state, s_keypoint, n_active, stream);
    if (rc != EKS_OK) return rc;
  }
  return EKS_OK;
}

int eks_adam_prepare(const eks_dims_t* d, const float* y, const double* A, int32_t n_blocks, void* workspace,
                     size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (n_blocks <= 0) return EKS_ERR_SHAPE;
  if (!y || !A) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  if (!(d->flags & EKS_FLAG_DIAG_MODEL) || !diag_lag_adam_ok(d->n_frames, d->n_keypoints, d->state_dim, n_blocks))
    return EKS_ERR_UNSUPPORTED;
  if (workspace_bytes < diag_nll_workspace_bytes(d->n_frames, d->n_keypoints * d->state_dim, 1)) return EKS_ERR_WORKSPACE;
  return diag_lag_sums(*d, y, A, nullptr, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int32_t eks_adam_run_stride(const eks_dims_t* d, int32_t n_blocks) {
  if (check_dims(d) != EKS_OK || n_blocks <= 0) return 4;
  if (!(d->flags & EKS_FLAG_DIAG_MODEL)) return 4;
  if (diag_lag_adam_ok(d->n_frames, d->n_keypoints, d->state_dim, n_blocks)) return 4096;
  if (diag_nll_adam_persist_ok(d->n_frames, d->n_keypoints, d->state_dim, n_blocks)) return 64;
  return 16;
}

int eks_pupil_adam_run(const eks_dims_t* d, const float* y, const float* var, const double* m0,
                       const double* S0, const double* C, const double* latent_var, double lr,
                       double tol, int32_t safety_cap, int32_t n_iters, double* state, double* a,
                       double* q, double* da, double* dq, double* nll, double* dnll,
                       int32_t* n_active, void* workspace, size_t workspace_bytes,
                       eks_stream_t stream) {
  if (n_iters < 0) return EKS_ERR_SHAPE;
  if (d && d->state_dim != 3) return EKS_ERR_SHAPE;   // (diameter, com_x, com_y)
  if (!nll || !dnll) return EKS_ERR_NULL;
  if (check_dims(d) != EKS_OK) return check_dims(d);
  if (!y || !var || !m0 || !S0 || !C || !latent_var || !state || !a || !q || !da || !dq || !n_active) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  for (int it = 0; it < n_iters; ++it) {
    // loss + tangents + step in three launches where the smoothing-distribution form covers the shape (round 4)
    int rc = dense_wave_ar1_score_step(*d, y, var, m0, S0, C, latent_var, lr, tol, safety_cap, state, a, q, da, dq, nll,
                                       dnll, n_active, workspace, workspace_bytes,
                                       reinterpret_cast<hipStream_t>(stream));
    if (rc == EKS_OK) continue;
    if (rc != EKS_ERR_UNSUPPORTED) return rc;
    rc = eks_ar1_nll(d, y, var, m0, S0, C, a, q, da, dq, 2, nll, dnll, workspace, workspace_bytes,
                     stream);
    if (rc != EKS_OK) return rc;
    rc = eks_pupil_adam_step(d->n_keypoints, latent_var, nll, dnll, lr, tol, safety_cap, state, a, q,
                             da, dq, n_active, stream);
    if (rc != EKS_OK) return rc;
  }
  return EKS_OK;
}

size_t eks_ekf_smooth_workspace_bytes(const eks_dims_t* d, int32_t want_smoother) {
  if (check_dims(d) != EKS_OK) return 0;
  return ekf_smooth_workspace_bytes(d->n_frames, d->n_keypoints, want_smoother);
}

int eks_ekf_smooth(const eks_dims_t* d, int32_t n_data_keypoints, const float* y, const float* var,
                   const double* rconst, const double* m0, const double* S0, const double* A,
                   const double* Q, const double* s, const double* cams, int32_t n_cams,
                   double* xlin, int32_t max_sweeps, double tol, float* ms, float* Vs, double* nll,
                   double* info, void* workspace, size_t workspace_bytes, eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (!y || !m0 || !S0 || !A || !Q || !s || !cams || !xlin) return EKS_ERR_NULL;
  if (!var && !rconst) return EKS_ERR_NULL;
  if (ms && !Vs) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  const DenseModel M{m0, S0, A, nullptr, Q, s};
  return ekf_smooth(*d, n_data_keypoints, y, var, rconst, M, cams, n_cams, xlin, max_sweeps, tol, ms,
                    Vs, nll, info, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

size_t eks_ekf_affine_workspace_bytes(const eks_dims_t* d, int32_t want_smoother) {
  if (check_dims(d) != EKS_OK) return 0;
  if (d->state_dim < 1 || d->state_dim > 6) return 0;
  return ekf_affine_workspace_bytes(d->n_frames, d->n_keypoints, d->state_dim, want_smoother);
}

int eks_ekf_affine_sweep(const eks_dims_t* d, int32_t n_data_keypoints, const float* y, const float* var,
                         const double* rconst, const double* m0, const double* S0, const double* A,
                         const double* Q, const double* s, const double* jac, const double* off, double* xlin,
                         float* ms, float* Vs, double* nll, double* change, void* workspace, size_t workspace_bytes,
                         eks_stream_t stream) {
  const int rc = check_dims(d);
  if (rc != EKS_OK) return rc;
  if (!y || !m0 || !S0 || !A || !Q || !s || !xlin) return EKS_ERR_NULL;
  if (!var && !rconst) return EKS_ERR_NULL;
  if (ms && !Vs) return EKS_ERR_NULL;
  if (!workspace) return EKS_ERR_WORKSPACE;
  const DenseModel M{m0, S0, A, nullptr, Q, s};
  return ekf_affine_sweep(*d, n_data_keypoints, y, var, rconst, M, jac, off, xlin, ms, Vs, nll, change, workspace,
                          workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int eks_ensemble(int32_t n_models, int32_t n_cameras, int32_t n_frames, int32_t n_keypoints,
                 const float* markers, int32_t avg_mode, int32_t var_mode, float nan_replacement,
                 float* stats, eks_stream_t stream) {
  if (n_models <= 0 || n_cameras <= 0 || n_frames <= 0 || n_keypoints <= 0) return EKS_ERR_SHAPE;
  if (avg_mode < 0 || avg_mode > 1 || var_mode < 0 || var_mode > 1) return EKS_ERR_UNSUPPORTED;
  if (!markers || !stats) return EKS_ERR_NULL;
  return ensemble_stats(n_models, n_cameras, n_frames, n_keypoints, markers, avg_mode, var_mode,
                        nan_replacement, stats, reinterpret_cast<hipStream_t>(stream));
}

int eks_maha_inflate(int32_t n_keypoints, int32_t n_frames, int32_t n_views, int32_t n_latent,
                     const double* x, float* v, const double* W, const double* mu,
                     const int32_t* active, double epsilon, double threshold, double scalar,
                     double* maha, int32_t* n_inflated, eks_stream_t stream) {
  if (n_keypoints <= 0 || n_frames <= 0 || n_views <= 0 || n_latent <= 0) return EKS_ERR_SHAPE;
  if (!x || !v || !W || !mu || !n_inflated) return EKS_ERR_NULL;
  return maha_inflate(n_keypoints, n_frames, n_views, n_latent, x, v, W, mu, active, epsilon, threshold,
                      scalar, maha, n_inflated, reinterpret_cast<hipStream_t>(stream));
}

int eks_multicam_tables(int32_t n_views, int32_t n_frames, int32_t n_keypoints, int32_t state_dim,
                        const float* stats, const float* ev, const float* ms, const float* Vs,
                        const double* C, const double* mean, double* tables, double* latent,
                        eks_stream_t stream) {
  if (n_views <= 0 || n_frames <= 0 || n_keypoints <= 0 || state_dim <= 0) return EKS_ERR_SHAPE;
  if (!stats || !ev || !ms || !Vs || !C || !mean || !tables) return EKS_ERR_NULL;
  return multicam_tables(n_views, n_frames, n_keypoints, state_dim, stats, ev, ms, Vs, C, mean, tables, latent,
                         reinterpret_cast<hipStream_t>(stream));
}

int eks_warmup(uint32_t units, float* ms_per_unit) {
  // order = the bits of EKS_WARM_* (include/eks_hip.h)
  static void (*const touch[])() = {eks::touch_misc,       eks::touch_diag,       eks::touch_diag_nll,
                                    eks::touch_dense,      eks::touch_dense_wave, eks::touch_dense_wide,
                                    eks::touch_loss,       eks::touch_loss_ar1,   eks::touch_multicam};
  for (unsigned i = 0; i < sizeof(touch) / sizeof(touch[0]); ++i) {
    if (ms_per_unit) ms_per_unit[i] = 0.f;
    if (!(units & (1u << i))) continue;
    const auto t0 = std::chrono::steady_clock::now();
    touch[i]();
    if (ms_per_unit)
      ms_per_unit[i] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (units & EKS_WARM_DIAG_NLL) eks::touch_lag_adam();        // (the search's own unit rides on the NLL bit)
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? EKS_OK : EKS_ERR_HIP_BASE - (int)e;
}

}  // extern "C"
