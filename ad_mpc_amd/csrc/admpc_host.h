// admpc_host.h -- what the host sides of the fleet units share: the device guard, the argument blocks of the two rollouts, and one
// declaration of every hidden function that one unit defines for another.  The defining unit includes this header too, so that the
// compiler holds each definition against its declaration.  Included by admpc_kernels.hip, admpc_step.hip, admpc_lane.hip,
// admpc_plant.hip, admpc_learn.hip, admpc_hyper.hip, admpc_quad.hip, admpc_quad_plant.hip, admpc_quad_fleet.hip, admpc_quad_learn.hip,
// admpc_quad_noise.hip, admpc_quad_ensemble.hip, admpc_quad_clusters.hip, admpc_quad_hyper.hip and admpc_quad_targets.hip.  The learning host
// side that admpc_learn.hip defines for admpc_quad_learn.hip and admpc_hyper.hip is declared in gp_fit_dev.h, next to the LearnArgs it
// speaks of; the search's host side that admpc_hyper.hip defines for admpc_quad_hyper.hip in gp_search_dev.h, next to its SearchGp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/admpc.h"
#include "../../include/admpc_fleet.h"
#include "../../include/admpc_lane.h"
#include "../../include/admpc_plant.h"
#include "../../include/admpc_learn.h"
#include "../../include/admpc_quad.h"
#include "../../include/admpc_quad_fleet.h"
#include "../../include/admpc_quad_learn.h"
#include "../../include/admpc_quad_noise.h"
#include "../../include/admpc_quad_targets.h"

// Every entry point runs on the solver's device and restores the caller's current device on return (a host with several GPUs
// keeps its own current device: torch allocations and default-stream work of the caller are not redirected).
struct DeviceGuard {
    int prev; bool switched; bool good;
    explicit DeviceGuard(int dev) : prev(-1), switched(false), good(true) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { good = hipSetDevice(dev) == hipSuccess; switched = good; }
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
    bool ok() const { return good; }
};

// what a control step writes, and the workspace it runs in (cost: null for the step on one global path)
struct StepOut {
    double *xbar, *ubar;
    int32_t* safe_count;
    double* prev_u;
    int32_t* has_valid;
    void* work;
    float* ack;
    int32_t *mode, *valid, *status;
    double* cost;
};

// admpc_rollout_lane_batch's arguments but T, traj and the stream: st holds the seven pose arrays, px .. steer
struct RolloutArgs {
    AdmpcSolver* s; const AdmpcPathBank* bank; const AdmpcLaneParams* lane; const AdmpcStepParams* prm;
    const AdmpcSolver* plant_model; const AdmpcPlantParams* plant;
    int B;
    const int32_t* path_of; int32_t* lane_idx;
    double* st[ADMPC_NX];
    StepOut out;
    double* tally; int32_t* counts;
};

// admpc_quad_rollout_batch's arguments but T, the records (traj_out, u_out) and the stream; noise: null, or the disturbances of
// admpc_quad_rollout_noise_batch (checked by it) with the vehicles' period counters; ens: null, or the clustered ensemble of
// admpc_quad_ensemble_rollout_batch, whose handles solve in place of s (s is its handle 0: the device, the horizon, the RTI mode), with
// route [B] and route_out (null or [T][B])
struct AdmpcQuadEnsemble;
struct QuadRolloutArgs {
    AdmpcQuadSolver* s; const AdmpcQuadTrajBank* bank; const AdmpcQuadPlantParams* plant;
    int over, B;
    const int32_t* traj_of; int32_t* idx;
    double *x, *xbar, *ubar, *yref, *yref_e, *cost;
    int32_t *status, *iters;
    double* tally; int32_t* counts;
    const AdmpcQuadNoiseParams* noise; uint64_t* noise_step;
    const AdmpcQuadEnsemble* ens; int32_t *route, *route_out;
};

struct QuadPlantArgs;       // quad_sim_dev.h: what one launch of a quadrotor plant kernel works on
struct QuadTargetArgs;      // quad_target_dev.h: the target state of such a launch

// the record slots of period t of a quadrotor rollout of B vehicles (traj_out: null or [T + 1][B][13], u_out: null or [T][B][4]): slot 0
// of traj_out is written by the first period; every period writes the state it leaves into the next slot
struct QuadRecordSlots { double *traj_pre, *traj_post, *u_out; };
inline QuadRecordSlots admpc_quad_record_slots(double* traj_out, double* u_out, int B, int t)
{
    const size_t slot = (size_t)B * ADMPC_QUAD_NX;
    return { t == 0 ? traj_out : nullptr, traj_out ? traj_out + (size_t)(t + 1) * slot : nullptr, u_out ? u_out + (size_t)t * B * ADMPC_QUAD_NU : nullptr };
}

#define ADMPC_HIDDEN extern "C" __attribute__((visibility("hidden")))

// admpc_kernels.hip: the thread-local message behind admpc_last_error(); a refusal (ADMPC_EINVAL, "who: what"); ADMPC_ENODEV unless
// `device` is one of the host's; the problem a handle solves and the device it lives on; the device copy of that problem, to be read and
// to be written; the horizon of a bank and its device; a bank's table (returns H)
ADMPC_HIDDEN int admpc_set_error(int code, const char* msg);
ADMPC_HIDDEN int admpc_refuse(const char* who, const char* what);
ADMPC_HIDDEN int admpc_device_check(int device);
ADMPC_HIDDEN const AdmpcConfig* admpc_solver_config(const AdmpcSolver* s, int* device);
ADMPC_HIDDEN const AdmpcConfig* admpc_solver_config_device(const AdmpcSolver* s);
ADMPC_HIDDEN AdmpcConfig* admpc_solver_config_device_rw(AdmpcSolver* s);
ADMPC_HIDDEN int admpc_path_bank_horizon(const AdmpcPathBank* bank, int* device);
ADMPC_HIDDEN int admpc_path_bank_table(const AdmpcPathBank* bank, int* device, int* K, double* dt, const void** desc, const double** cols);
// admpc_lane.hip, admpc_plant.hip, admpc_learn.hip: the refusals of a parameter block (`who` leads the message)
ADMPC_HIDDEN int admpc_lane_params_check(const char* who, const AdmpcLaneParams* lane, const int32_t* lane_idx);
ADMPC_HIDDEN int admpc_plant_params_check(const char* who, const AdmpcPlantParams* plant);
ADMPC_HIDDEN int admpc_observe_params_check(const char* who, const AdmpcObserveParams* obs);
// admpc_plant.hip: one launch of the plant kernel for checked arguments
ADMPC_HIDDEN int admpc_plant_launch(const AdmpcSolver* model, const AdmpcPlantParams* plant, int B, const float* ack, const int32_t* mode,
                                    double* const* st, const double* err, const int32_t* status, const int32_t* valid, double* tally,
                                    int32_t* counts, double* traj_pre, double* traj_post, void* stream);
// admpc_step.hip: the refusals of a rollout up to its arrays, those behind them (T, the plant's device), and one checked period
ADMPC_HIDDEN int admpc_rollout_check_step(const RolloutArgs& a);
ADMPC_HIDDEN int admpc_rollout_check_run(const RolloutArgs& a, int T);
ADMPC_HIDDEN int admpc_rollout_enqueue(const RolloutArgs& a, double* traj_pre, double* traj_post, void* stream);
// admpc_quad.hip: the device copy of a quadrotor handle's problem, which admpc_quad_learn.hip reads (observe) and writes (install), and
// the n_gp the handle was created with (n_gp may be NULL); next to admpc_quad_solver_info of include/admpc_quad_fleet.h
ADMPC_HIDDEN AdmpcQuadConfig* admpc_quad_solver_config_device(const AdmpcQuadSolver* s, int* n_gp);
// admpc_quad_plant.hip: the refusals of the quadrotor's plant parameters; the arguments of a plant-only step (a period of a rollout
// sets its own pointers behind it); one launch of a plant kernel for filled arguments, B > 0, on the current device -- noise: null, or
// checked disturbances with the period counters; g: null, or the target state of admpc_quad_targets.hip
ADMPC_HIDDEN int admpc_quad_plant_params_check(const char* who, const AdmpcQuadPlantParams* plant);
ADMPC_HIDDEN void admpc_quad_plant_fill(QuadPlantArgs& a, const AdmpcQuadPlantParams* plant, int B, const double* u, long long u_stride, double* x);
ADMPC_HIDDEN int admpc_quad_plant_launch(const QuadPlantArgs& a, const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, const QuadTargetArgs* g, void* stream);
// admpc_quad_fleet.hip: the refusals of a rollout up to those of its arrays (under admpc_quad_rollout_batch's name), and one checked period
ADMPC_HIDDEN int admpc_quad_rollout_check(const QuadRolloutArgs& a, int T);
ADMPC_HIDDEN int admpc_quad_rollout_enqueue(const QuadRolloutArgs& a, double* traj_pre, double* traj_post, double* u_out, int32_t* route_out, void* stream);
// admpc_quad_fleet.hip, admpc_quad_learn.hip: a whole rollout and a whole observed rollout behind their arguments' block, refusals and
// no-ops included (under the names of admpc_quad_rollout_batch and admpc_quad_rollout_observe_batch).  samples_step: what the samples
// pointer advances by per period, 0 for every entry but the logged rollout of admpc_quad_clusters.hip ([T][B][14]: B * 14).  The
// observed run's refusals alone, for that entry, which has one more behind them: 0 also where B == 0 or T == 0
ADMPC_HIDDEN int admpc_quad_rollout_run(const QuadRolloutArgs& a, int T, double* traj_out, double* u_out, void* stream);
ADMPC_HIDDEN int admpc_quad_rollout_observe_check(const QuadRolloutArgs& a, int T, const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                                  const double* prev, const double* samples, const double* bins, const int32_t* dropped);
ADMPC_HIDDEN int admpc_quad_rollout_observe_run(const QuadRolloutArgs& a, int T, double* traj_out, double* u_out, const AdmpcQuadSolver* model,
                                                const AdmpcQuadObserveParams* obs, double* prev, double* samples, long long samples_step,
                                                double* bins, int32_t* dropped, void* stream);
// admpc_quad_noise.hip: the refusals of the disturbances (plant: null, or the plant whose u_min motor_noise is held against)
ADMPC_HIDDEN int admpc_quad_noise_params_check(const char* who, const AdmpcQuadNoiseParams* noise, const AdmpcQuadPlantParams* plant);
// admpc_quad_targets.hip: the refusals of the target parameters
ADMPC_HIDDEN int admpc_quad_target_params_check(const char* who, const AdmpcQuadTargetParams* t);
// admpc_quad_learn.hip: the refusals of the quadrotor's observe parameters; the two launches of an observation for checked arguments,
// B > 0, on the model's device -- with ens the bin launch is the ensemble's, all clusters at once; nsub: null, or the sub-steps every
// vehicle flew of its period ([B]: the observation over the flown time of include/admpc_quad_targets.h)
ADMPC_HIDDEN int admpc_quad_observe_params_check(const char* who, const AdmpcQuadObserveParams* obs);
ADMPC_HIDDEN int admpc_quad_observe_launch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs,
                                           const AdmpcQuadEnsemble* ens, int B, const double* u, long long u_stride, const double* x, double* prev,
                                           const int32_t* nsub, double* samples, double* bins, int32_t* dropped, void* stream);
// admpc_quad_learn.hip: the bin launch of an observation alone (the second of the two above, without an ensemble), and the latch, which
// admpc_quad_targets.hip launches too, both for checked arguments, B > 0, on the current device
ADMPC_HIDDEN int admpc_quad_bin_launch(const AdmpcQuadObserveParams* obs, int B, const double* samples, double* bins, int32_t* dropped, void* stream);
ADMPC_HIDDEN int admpc_quad_latch_launch(int B, const double* x, double* prev, void* stream);
// admpc_quad_ensemble.hip: the handles of an ensemble (returns K); what admpc_quad_clusters.hip and admpc_quad_hyper.hip need of one (its
// device centroids to be written, its features, whether it learns and under which blocks, the device copy of its regressors, its search
// slot); one launch of its route kernel (route_out: null or [B]) and one of its bin kernel, B > 0, on its device
struct LearnGp;                                 // gp_fit_dev.h: one regressor as the learning kernels read it
// what admpc_quad_hyper.hip keeps in an ensemble: the device copy of the search descriptors (null until the first
// admpc_quad_ensemble_set_search; the object frees it), and what the K blocks of the last one agree in, with their largest candidate count
struct QuadEnsembleSearch {
    void* d_desc;
    int set, grid, rounds, cmax;
    double shrink;
};
struct QuadEnsembleView {
    int device, K, n_feat, feat[3], learns, n_gp;
    double* cent;                               // device [K][n_feat]
    const AdmpcQuadObserveParams* obs;          // host [K] (learns)
    const LearnGp* gp;                          // device [K][ADMPC_QUAD_GP_MAX] (learns)
    QuadEnsembleSearch* search;                 // the object's own, to be written by admpc_quad_ensemble_set_search
};
ADMPC_HIDDEN int admpc_quad_ensemble_handles(const AdmpcQuadEnsemble* e, AdmpcQuadSolver* const** solvers);
ADMPC_HIDDEN void admpc_quad_ensemble_view(const AdmpcQuadEnsemble* e, QuadEnsembleView* v);
ADMPC_HIDDEN int admpc_quad_ensemble_route_launch(const AdmpcQuadEnsemble* e, int B, const double* yref, int32_t* route, int32_t* route_out, void* stream);
ADMPC_HIDDEN int admpc_quad_ensemble_bin_launch(const AdmpcQuadEnsemble* e, int B, const double* samples, double* bins, int32_t* dropped, void* stream);
