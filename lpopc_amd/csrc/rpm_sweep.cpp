// rpm_sweep.cpp — rpm_sweep_*: the batched device solver (rpm_ipm_*, row f-2) over several GPUs from ONE process.  The B
// independent instances of one transcription (the MPC sweep of BASELINE config 5) are dealt to the listed devices in contiguous
// shares; every device has its own engine and solver, a call runs them side by side on a host thread each (the solver's loop
// blocks on its stream's counters).  Nothing crosses between devices: an instance's result is what a single engine computes for
// it.  No reference counterpart (lpopc hands one NLP to Ipopt, Core/LpNLPSolver.cpp:13-53).  Host only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "rpm_device_restore.hpp"
#include "rpm_engine.hpp"

struct rpm_sweep {
  std::vector<rpm_engine*> eng;
  std::vector<rpm_ipm*> ipm;
  std::vector<int> dev, first, count;   // device, first instance and number of instances of every share
  int B = 0, n = 0, m = 0;
  std::string err;
};

static std::string g_sweep_create_error;

static int sfail(rpm_sweep* s, size_t r, int rc, const char* why) {
  s->err = "share " + std::to_string(r) + " (device " + std::to_string(s->dev[r]) + "): " + why;
  return rc;
}

// fn(r) on every share side by side, each on a host thread of its own with the share's device current (the current device is per
// host thread), share 0 on the caller's; the caller's current device is put back.  The first share whose fn failed is reported
// with why(r).
template <class Fn, class Why>
static int for_each_share(rpm_sweep* s, Fn fn, Why why) {
  const size_t N = s->eng.size();
  rpm::DeviceRestore restore;
  std::vector<int> rcs(N, RPM_OK);
  auto run = [&](size_t r) {
    (void)hipSetDevice(s->dev[r]);
    rcs[r] = fn(r);
  };
  std::vector<std::thread> th;
  for (size_t r = 1; r < N; ++r) th.emplace_back(run, r);
  run(0);
  for (std::thread& t : th) t.join();
  for (size_t r = 0; r < N; ++r)
    if (rcs[r]) return sfail(s, r, rcs[r], why(r));
  return RPM_OK;
}

extern "C" {

void rpm_sweep_destroy(rpm_sweep* s) {
  if (!s) return;
  for (size_t r = 0; r < s->eng.size(); ++r) {
    if (r < s->ipm.size() && s->ipm[r]) rpm_ipm_destroy(s->ipm[r]);
    if (s->eng[r]) rpm_destroy(s->eng[r]);
  }
  delete s;
}

int rpm_sweep_create(const rpm_problem_desc* desc, int n_devices, const int* device_ids, rpm_sweep** out) {
  if (!out) return RPM_E_INVALID;
  *out = nullptr;
  if (!desc || !device_ids || n_devices < 1 || n_devices > RPM_GROUP_MAX || desc->n_instances < n_devices) {
    g_sweep_create_error = "rpm_sweep_create: need 1 .. RPM_GROUP_MAX devices and at least one instance per device";
    return RPM_E_INVALID;
  }
  rpm_sweep* s = new (std::nothrow) rpm_sweep();
  if (!s) return RPM_E_INVALID;
  s->B = desc->n_instances;
  for (int r = 0; r < n_devices; ++r) {
    const int i0 = int((long long)s->B * r / n_devices), i1 = int((long long)s->B * (r + 1) / n_devices);
    rpm_problem_desc d = *desc;
    d.n_instances = i1 - i0;
    rpm_engine* e = nullptr;
    int rc = rpm_create(&d, &e);
    if (rc == RPM_OK) {
      s->eng.push_back(e);
      rc = rpm_device_init(e, device_ids[r]);
    }
    rpm_ipm* p = nullptr;
    if (rc == RPM_OK) rc = rpm_ipm_create(e, &p);
    if (rc != RPM_OK) {
      g_sweep_create_error = std::string("rpm_sweep_create, device ") + std::to_string(device_ids[r]) + ": " + rpm_last_error(e);
      rpm_sweep_destroy(s);
      return rc;
    }
    s->ipm.push_back(p);
    s->dev.push_back(device_ids[r]);
    s->first.push_back(i0);
    s->count.push_back(i1 - i0);
  }
  int nnz_j = 0, nnz_h = 0, style = 0;
  rpm_get_nlp_info(s->eng[0], &s->n, &s->m, &nnz_j, &nnz_h, &style);
  *out = s;
  return RPM_OK;
}

const char* rpm_sweep_last_error(const rpm_sweep* s) { return s ? s->err.c_str() : g_sweep_create_error.c_str(); }
int rpm_sweep_size(const rpm_sweep* s) { return s ? int(s->eng.size()) : 0; }
rpm_engine* rpm_sweep_engine(rpm_sweep* s, int share) { return (s && share >= 0 && share < int(s->eng.size())) ? s->eng[size_t(share)] : nullptr; }
rpm_ipm* rpm_sweep_solver(rpm_sweep* s, int share) { return (s && share >= 0 && share < int(s->ipm.size())) ? s->ipm[size_t(share)] : nullptr; }
int rpm_sweep_share(const rpm_sweep* s, int share, int* first_instance, int* n_instances) {
  if (!s || share < 0 || share >= int(s->eng.size())) return RPM_E_INVALID;
  if (first_instance) *first_instance = s->first[size_t(share)];
  if (n_instances) *n_instances = s->count[size_t(share)];
  return RPM_OK;
}

int rpm_sweep_set_option(rpm_sweep* s, const char* key, double value) {
  if (!s || !key) return RPM_E_INVALID;
  for (size_t r = 0; r < s->ipm.size(); ++r) {
    const int rc = rpm_ipm_set_option(s->ipm[r], key, value);
    if (rc) return sfail(s, r, rc, rpm_ipm_last_error(s->ipm[r]));
  }
  return RPM_OK;
}

int rpm_sweep_set_bounds(rpm_sweep* s, int instance, const double* x_l, const double* x_u) {
  if (!s || instance < 0 || instance >= s->B) return RPM_E_INVALID;
  for (size_t r = 0; r < s->ipm.size(); ++r)
    if (instance < s->first[r] + s->count[r]) {
      rpm::DeviceRestore restore;
      (void)hipSetDevice(s->dev[r]);
      const int rc = rpm_ipm_set_bounds(s->ipm[r], instance - s->first[r], x_l, x_u);
      return rc ? sfail(s, r, rc, rpm_ipm_last_error(s->ipm[r])) : RPM_OK;
    }
  return RPM_E_INVALID;
}

/* x: B x n (starting points in, solutions out), lambda: B x m or NULL; per instance, any may be NULL: objective, status,
 * iteration count, scaled KKT error — as rpm_ipm_solve, over all shares at once */
int rpm_sweep_solve(rpm_sweep* s, double* x, double* lambda, double* obj, int* status, int* iterations, double* kkt_error) {
  if (!s || !x) return RPM_E_INVALID;
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_ipm_solve(s->ipm[r], x + i0 * s->n, lambda ? lambda + i0 * s->m : nullptr, obj ? obj + i0 : nullptr,
                             status ? status + i0 : nullptr, iterations ? iterations + i0 : nullptr, kkt_error ? kkt_error + i0 : nullptr);
      },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* rpm_ipm_solve_warm over all shares at once: x B x n, lambda B x m (required), z_L / z_U B x n (both or neither), all in/out */
int rpm_sweep_solve_warm(rpm_sweep* s, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status, int* iterations,
                         double* kkt_error) {
  if (!s) return RPM_E_INVALID;
  if (!x || !lambda || (!z_L != !z_U)) {
    s->err = (!x || !lambda) ? "rpm_sweep_solve_warm: x and lambda are required" : "rpm_sweep_solve_warm: z_L and z_U are given together or both NULL";
    return RPM_E_INVALID;
  }
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_ipm_solve_warm(s->ipm[r], x + i0 * s->n, lambda + i0 * s->m, z_L ? z_L + i0 * s->n : nullptr,
                                  z_U ? z_U + i0 * s->n : nullptr, obj ? obj + i0 : nullptr, status ? status + i0 : nullptr,
                                  iterations ? iterations + i0 : nullptr, kkt_error ? kkt_error + i0 : nullptr);
      },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* rpm_ipm_get_bound_multipliers of every share: z_L, z_U B x n */
int rpm_sweep_get_bound_multipliers(rpm_sweep* s, double* z_L, double* z_U) {
  if (!s) return RPM_E_INVALID;
  if (!z_L || !z_U) {
    s->err = "rpm_sweep_get_bound_multipliers: z_L or z_U is NULL";
    return RPM_E_INVALID;
  }
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_ipm_get_bound_multipliers(s->ipm[r], z_L + i0 * s->n, z_U + i0 * s->n);
      },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* rpm_ipm_sensitivities of every share: dx B x n_par x n, dlambda B x n_par x m or NULL, delta_w and info B or NULL.  The list is
 * checked by every share's solver (they share one plan); n_par is needed here for the shares' offsets. */
int rpm_sweep_sensitivities(rpm_sweep* s, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, int* info) {
  if (!s) return RPM_E_INVALID;
  if (!var_index || !dx || n_par < 1) {
    s->err = (!var_index || !dx) ? "rpm_sweep_sensitivities: var_index or dx is NULL" : "rpm_sweep_sensitivities: n_par must be at least 1";
    return RPM_E_INVALID;
  }
  const size_t P = size_t(n_par);
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_ipm_sensitivities(s->ipm[r], n_par, var_index, dx + i0 * P * s->n, dlambda ? dlambda + i0 * P * s->m : nullptr,
                                     delta_w ? delta_w + i0 : nullptr, info ? info + i0 : nullptr);
      },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* rpm_ipm_constant_sensitivities of every share, laid out as rpm_sweep_sensitivities lays its results out. */
int rpm_sweep_constant_sensitivities(rpm_sweep* s, int n_par, const int* const_index, double* dx, double* dlambda, double* delta_w,
                                     int* info) {
  if (!s) return RPM_E_INVALID;
  if (!const_index || !dx || n_par < 1) {
    s->err = (!const_index || !dx) ? "rpm_sweep_constant_sensitivities: const_index or dx is NULL" : "rpm_sweep_constant_sensitivities: n_par must be at least 1";
    return RPM_E_INVALID;
  }
  const size_t P = size_t(n_par);
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_ipm_constant_sensitivities(s->ipm[r], n_par, const_index, dx + i0 * P * s->n, dlambda ? dlambda + i0 * P * s->m : nullptr,
                                              delta_w ? delta_w + i0 : nullptr, info ? info + i0 : nullptr);
      },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* The mesh-error estimate of the whole sweep (rpm_solution_error_batch on every share, side by side).  x: B x n; instance_mask:
 * B or NULL; any result may be NULL: interval_error B x KT, rel_err_max RT, rel_err B x RT, nonfinite B.  rel_err_max is the
 * element-wise maximum of the shares' blocks (a maximum: what one engine holding all B instances returns, bit for bit); a share
 * whose instances are all excluded contributes nothing to it. */
int rpm_sweep_solution_error(rpm_sweep* s, const double* x, const int* instance_mask, double* interval_error, double* rel_err_max,
                             double* rel_err, int* nonfinite) {
  if (!s || !x) return RPM_E_INVALID;
  const size_t N = s->eng.size();
  int KT = 0;
  long long RT = 0;
  rpm_solution_error_batch_sizes(s->eng[0], &KT, &RT);
  std::vector<char> included(N, 1);
  if (instance_mask) {
    bool any = false;
    for (size_t r = 0; r < N; ++r) {
      included[r] = 0;
      for (int b = 0; b < s->count[r]; ++b) included[r] = included[r] || instance_mask[s->first[r] + b] != 0;
      any = any || included[r];
    }
    if (!any && rel_err_max) {
      s->err = "rpm_sweep_solution_error: rel_err_max asked for, but instance_mask excludes every instance";
      return RPM_E_INVALID;
    }
  }
  std::vector<std::vector<double>> part(N);
  const int rc = for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        const bool want_max = rel_err_max && included[r];
        if (want_max) part[r].resize(size_t(RT));
        return rpm_solution_error_batch(s->eng[r], x + i0 * s->n, instance_mask ? instance_mask + i0 : nullptr,
                                        interval_error ? interval_error + i0 * KT : nullptr, want_max ? part[r].data() : nullptr,
                                        rel_err ? rel_err + i0 * size_t(RT) : nullptr, nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(s->eng[r]); });
  if (rc) return rc;
  if (rel_err_max) {
    bool has = false;
    for (size_t r = 0; r < N; ++r) {
      if (!included[r]) continue;
      for (long long i = 0; i < RT; ++i) rel_err_max[i] = has ? rpm::mesh_err_max(rel_err_max[i], part[r][size_t(i)]) : part[r][size_t(i)];
      has = true;
    }
  }
  return RPM_OK;
}

/* rpm_carry_solution_batch on every share, side by side: x_from B x from.n, x_to B x to.n, nonfinite B or NULL.  The two sweeps
 * must deal their instances alike (same devices, same shares). */
int rpm_sweep_carry_solution(rpm_sweep* from, rpm_sweep* to, const double* x_from, double* x_to, int* nonfinite) {
  if (!from) return RPM_E_INVALID;
  if (!to || !x_from || !x_to) {
    from->err = !to ? "rpm_sweep_carry_solution: the target sweep is NULL" : "rpm_sweep_carry_solution: x_from or x_to is NULL";
    return RPM_E_INVALID;
  }
  if (from->B != to->B || from->dev != to->dev || from->count != to->count) {
    from->err = "rpm_sweep_carry_solution: the sweeps have different shares (devices or instance counts)";
    return RPM_E_INVALID;
  }
  return for_each_share(
      from,
      [&](size_t r) {
        const size_t i0 = size_t(from->first[r]);
        return rpm_carry_solution_batch(from->eng[r], to->eng[r], x_from + i0 * from->n, x_to + i0 * to->n, nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(from->eng[r]); });
}

/* rpm_carry_multipliers_batch on every share, side by side: x_from B x from.n, lambda_from B x from.m, lambda_to B x to.m */
int rpm_sweep_carry_multipliers(rpm_sweep* from, rpm_sweep* to, const double* x_from, const double* lambda_from, double* lambda_to,
                                int* nonfinite) {
  if (!from) return RPM_E_INVALID;
  if (!to || !x_from || !lambda_from || !lambda_to) {
    from->err = !to ? "rpm_sweep_carry_multipliers: the target sweep is NULL" : "rpm_sweep_carry_multipliers: x_from, lambda_from or lambda_to is NULL";
    return RPM_E_INVALID;
  }
  if (from->B != to->B || from->dev != to->dev || from->count != to->count) {
    from->err = "rpm_sweep_carry_multipliers: the sweeps have different shares (devices or instance counts)";
    return RPM_E_INVALID;
  }
  return for_each_share(
      from,
      [&](size_t r) {
        const size_t i0 = size_t(from->first[r]);
        return rpm_carry_multipliers_batch(from->eng[r], to->eng[r], x_from + i0 * from->n, lambda_from + i0 * from->m,
                                           lambda_to + i0 * to->m, nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(from->eng[r]); });
}

/* rpm_shift_plan_batch on every share, side by side: dt B x n_phases, x / z B x n, lambda B x m, nonfinite B or NULL */
int rpm_sweep_shift_plan(rpm_sweep* s, const double* dt, const double* x, double* x_out, const double* lambda, double* lambda_out,
                         const double* z_L, const double* z_U, double* z_L_out, double* z_U_out, int* nonfinite) {
  if (!s) return RPM_E_INVALID;
  if (!dt || !x || !x_out) {
    s->err = "rpm_sweep_shift_plan: dt, x or x_out is NULL";
    return RPM_E_INVALID;
  }
  const size_t P = size_t(s->eng[0]->e.P);
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        auto at = [&](auto* p, size_t stride) { return p ? p + i0 * stride : nullptr; };
        return rpm_shift_plan_batch(s->eng[r], dt + i0 * P, x + i0 * s->n, x_out + i0 * s->n, at(lambda, size_t(s->m)),
                                    at(lambda_out, size_t(s->m)), at(z_L, size_t(s->n)), at(z_U, size_t(s->n)), at(z_L_out, size_t(s->n)),
                                    at(z_U_out, size_t(s->n)), nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(s->eng[r]); });
}

/* rpm_sample_plan_batch on every share, side by side: x B x n, times B x n_times, out B x (nx + nu) x n_times, nonfinite B or NULL */
int rpm_sweep_sample_plan(rpm_sweep* s, int phase, const double* x, int n_times, const double* times, double* out, int* nonfinite) {
  if (!s) return RPM_E_INVALID;
  if (!x || !times || !out || n_times < 1 || phase < 0 || phase >= s->eng[0]->e.P) {
    s->err = (!x || !times || !out) ? "rpm_sweep_sample_plan: x, times or out is NULL"
                                    : (n_times < 1 ? "rpm_sweep_sample_plan: n_times must be at least 1" : "rpm_sweep_sample_plan: the phase index is out of range");
    return RPM_E_INVALID;
  }
  const rpm::PhaseHost& p = s->eng[0]->e.ph[size_t(phase)];
  const size_t nt = size_t(n_times), block = size_t(p.nx + p.nu) * nt;
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_sample_plan_batch(s->eng[r], phase, x + i0 * s->n, n_times, times + i0 * nt, out + i0 * block,
                                     nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(s->eng[r]); });
}

/* rpm_rollout_batch on every share, side by side: x B x n, t_start (or NULL) and dt B, state0 (or NULL) and state_out B x nx, traj
 * B x (n_steps + 1) x nx or NULL, nonfinite B or NULL */
int rpm_sweep_rollout(rpm_sweep* s, int phase, const double* x, const double* t_start, const double* dt, int n_steps, int hold,
                      const double* state0, double* state_out, double* traj, int* nonfinite) {
  if (!s) return RPM_E_INVALID;
  if (!x || !dt || !state_out || n_steps < 1 || n_steps > 65536 || phase < 0 || phase >= s->eng[0]->e.P) {
    s->err = (!x || !dt || !state_out) ? "rpm_sweep_rollout: x, dt or state_out is NULL"
                                       : ((n_steps < 1 || n_steps > 65536) ? "rpm_sweep_rollout: n_steps must be 1 ... 65536" : "rpm_sweep_rollout: the phase index is out of range");
    return RPM_E_INVALID;
  }
  const size_t nx = size_t(s->eng[0]->e.ph[size_t(phase)].nx), row = (size_t(n_steps) + 1) * nx;
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_rollout_batch(s->eng[r], phase, x + i0 * s->n, t_start ? t_start + i0 : nullptr, dt + i0, n_steps, hold,
                                 state0 ? state0 + i0 * nx : nullptr, state_out + i0 * nx, traj ? traj + i0 * row : nullptr,
                                 nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(s->eng[r]); });
}

/* rpm_ipm_set_initial_states of every share: state0 B x nx of the phase */
int rpm_sweep_set_initial_states(rpm_sweep* s, int phase, const double* state0) {
  if (!s) return RPM_E_INVALID;
  if (!state0 || phase < 0 || phase >= s->eng[0]->e.P) {
    s->err = !state0 ? "rpm_sweep_set_initial_states: state0 is NULL" : "rpm_sweep_set_initial_states: the phase index is out of range";
    return RPM_E_INVALID;
  }
  const size_t nx = size_t(s->eng[0]->e.ph[size_t(phase)].nx);
  return for_each_share(
      s, [&](size_t r) { return rpm_ipm_set_initial_states(s->ipm[r], phase, state0 + size_t(s->first[r]) * nx); },
      [&](size_t r) { return rpm_ipm_last_error(s->ipm[r]); });
}

/* rpm_nlp2op_batch on every share, side by side: x B x n, lambda B x m, out B x EB, nonfinite B or NULL */
int rpm_sweep_nlp2op(rpm_sweep* s, const double* x, const double* lambda, double* out, int* nonfinite) {
  if (!s) return RPM_E_INVALID;
  if (!x || !lambda || !out) {
    s->err = "rpm_sweep_nlp2op: x, lambda or out is NULL";
    return RPM_E_INVALID;
  }
  long long EB = 0;
  rpm_nlp2op_batch_layout(s->eng[0], 0, nullptr, &EB);
  return for_each_share(
      s,
      [&](size_t r) {
        const size_t i0 = size_t(s->first[r]);
        return rpm_nlp2op_batch(s->eng[r], x + i0 * s->n, lambda + i0 * s->m, out + i0 * size_t(EB), nonfinite ? nonfinite + i0 : nullptr);
      },
      [&](size_t r) { return rpm_last_error(s->eng[r]); });
}

/* totals over the shares of the last solve: batched iterations (the largest share's count), factorisations and trial points (sums) */
int rpm_sweep_get_stats(rpm_sweep* s, int* iterations, int* factorizations, int* trial_points) {
  if (!s) return RPM_E_INVALID;
  int it = 0, fa = 0, tr = 0;
  for (rpm_ipm* p : s->ipm) {
    int a = 0, b = 0, c = 0;
    const int rc = rpm_ipm_get_stats(p, &a, &b, &c);
    if (rc) return rc;
    it = std::max(it, a); fa += b; tr += c;
  }
  if (iterations) *iterations = it;
  if (factorizations) *factorizations = fa;
  if (trial_points) *trial_points = tr;
  return RPM_OK;
}

}  // extern "C"
