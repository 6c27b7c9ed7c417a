/* dtrl.h -- C ABI of the MI355X batched rollout engine (libdtrl.so).
 *
 * The reference (xbpeng/DeepTerrainRL) has no FFI; its seam is the C++ virtual interface between the scenario
 * drivers (cScenarioTrain::ExpHelper, cOptScenarioPoliEval::EvalHelper) and ONE environment object. This header is
 * that seam for a BATCH of environments: every entry point names the reference interface it replaces
 * (file:line relative to the reference repo root). All buffers are caller-owned host memory; no torch types.
 * A batch handle is driven from one host thread (like one reference scenario object, scenarios/ScenarioTrain.cpp:467-475).
 *
 * Error behaviour mirrors the reference's bool-return + message convention (no exceptions): every call returns a
 * dtrl_status; dtrl_last_error() gives the message. There is NO CPU fallback: dtrl_create fails with
 * DTRL_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef DTRL_H_
#define DTRL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dtrl_batch dtrl_batch;

typedef enum {
	DTRL_OK = 0,
	DTRL_ERR_ARG = 1,        /* bad argument / arg file */
	DTRL_ERR_IO = 2,         /* missing or malformed data file */
	DTRL_ERR_NO_DEVICE = 3,  /* no usable HIP device (product never falls back to CPU) */
	DTRL_ERR_DEVICE = 4,     /* HIP runtime error */
	DTRL_ERR_UNSUPPORTED = 5,
	DTRL_ERR_CAPACITY = 6
} dtrl_status;

/* flags returned by dtrl_get_flags */
#define DTRL_FLAG_FALLEN 1u
#define DTRL_FLAG_STUMBLED 2u
#define DTRL_FLAG_NEW_CYCLE 4u
#define DTRL_FLAG_STATE_SHIFT 8

/* tuple flag bits: learning/MACETrainer.h:11-17 (eFlagFail, eFlagExpCritic, eFlagExpActor) */
#define DTRL_TUPLE_FAIL 1u
#define DTRL_TUPLE_EXP_CRITIC 2u
#define DTRL_TUPLE_EXP_ACTOR 4u

/* Build a batch of num_envs environments from reference-format arguments.
 * Replaces: cArgParser(argv) + AppendArgs(-arg_file) (optimizer/Main.cpp:19-32, util/ArgParser.cpp:42-108) and, per env,
 * cScenarioExp/cScenarioPoliEval::ParseArgs + Init (scenarios/ScenarioSimChar.cpp:76-119, scenarios/ScenarioExp.cpp:31-61),
 * i.e. cScenarioTrain::BuildScenePool (scenarios/ScenarioTrain.cpp:197-222).
 * Relative paths inside the arg file resolve against the value of "-data_root=" if given, else the current directory
 * (the reference is run from its repo root). Extra keys understood: -data_root=, -terrain_seed= (env i uses seed+i),
 * -rand_seed= (exploration streams), -global_env_offset= (first global env id of this shard),
 * -physics_precision= f64 | f32: a CHECK, not a switch -- libdtrl.so computes in fp64 (default; the parity-tested product), libdtrl_f32.so is the same
 * source built with float arithmetic (opt-in; Bullet's own state is float, premake4.lua:115-124; distribution-level parity only) behind this same ABI
 * (doubles in, doubles out); each library fails dtrl_create with DTRL_ERR_ARG when asked for the other precision.
 * device_id < 0 selects the current HIP device. */
dtrl_status dtrl_create(const char* const* argv, int argc, int num_envs, int device_id, dtrl_batch** out);

/* Replaces: cScenario::Clear/Shutdown + destructor (scenarios/Scenario.h:15-23). */
dtrl_status dtrl_destroy(dtrl_batch* b);

/* Replaces: cScenarioExp::Reset / cScenarioPoliEval::Reset on the listed envs (scenarios/ScenarioSimChar.cpp:121-132,
 * scenarios/ScenarioExp.cpp:63-73). env_ids == NULL resets all. terrain_seeds != NULL re-seeds those envs' ground RNG
 * first (cScenarioPoliEval::SetRandSeed, scenarios/ScenarioPoliEval.cpp:153-160). */
dtrl_status dtrl_reset(dtrl_batch* b, const int32_t* env_ids, int n, const uint64_t* terrain_seeds);

/* Replaces: cScenarioExp::Update(dt) / cScenarioPoliEval::Update(dt) on every env
 * (scenarios/ScenarioExp.cpp:83-98, scenarios/ScenarioPoliEval.cpp:110-125): num_update_steps iterations of the loop at
 * scenarios/ScenarioSimChar.cpp:162-173, then fall handling (tuple + reset). dt is normally 1/30. */
dtrl_status dtrl_step(dtrl_batch* b, double dt);

/* dtrl_step split in two, so the caller can overlap its own GPU work (e.g. the trainer: the reference's env threads and trainer
 * run concurrently, scenarios/ScenarioTrain.cpp:100-115) with the frame kernel: dtrl_step_begin queues the frame launch on the
 * engine's stream and returns; dtrl_step_end waits for it and performs the frame-boundary host work (terrain windows, resets).
 * dtrl_step(dt) == dtrl_step_begin(dt); dtrl_step_end(). No other call on the batch is allowed between the two. */
dtrl_status dtrl_step_begin(dtrl_batch* b, double dt);
dtrl_status dtrl_step_end(dtrl_batch* b);

/* Finer grain: n iterations of the loop body only (no end-of-frame fall handling); used by parity tests and to count in
 * env-steps. The step length is (1/30)/num_update_steps. */
dtrl_status dtrl_step_updates(dtrl_batch* b, int n);

/* Asynchronous variant of dtrl_step for throughput runs: enqueue `frames` outer frames back-to-back on the batch's HIP
 * stream, doing the per-frame host work (terrain window slides, fall resets) between launches. Returns after the last
 * frame completed. */
dtrl_status dtrl_run_frames(dtrl_batch* b, int frames, double dt);

/* Replaces: cNNController::LoadNet + LoadModel + LoadScale (sim/NNController.cpp:49-91; learning/NeuralNet.cpp:81-215)
 * and cNeuralNet::CopyModel pushes from the trainer (learning/NeuralNetLearner.cpp:85-89). weights: flat float32 in Caffe
 * blob order of the deploy prototxt named by -policy_net= (W then b per layer). Offsets/scales follow
 * learning/NeuralNet.cpp:977-986,1027-1036. n must equal dtrl_policy_num_params().  * With -char_ctrl= dog_cacla the net is the CACLA ACTOR (cBaseControllerCacla::CopyActorNet, sim/BaseControllerCacla.cpp:67-75): weights in the actor
 * deploy net's blob order, output normalisers of its 29 outputs. */
dtrl_status dtrl_set_policy(dtrl_batch* b, const float* weights, size_t n, const double* in_off, const double* in_scale, const double* out_off, const double* out_scale);
dtrl_status dtrl_policy_num_params(const dtrl_batch* b, size_t* n);

/* Replaces: cNNController::BuildNNOutputOffsetScale (sim/BaseControllerMACE.cpp:75-113, sim/DogControllerMACE.cpp:93-99);
 * used by cScenarioTrain::SetupTrainerOutputOffsetScale (scenarios/ScenarioTrain.cpp:322-338). */
dtrl_status dtrl_build_output_offset_scale(const dtrl_batch* b, double* out_off, double* out_scale);

/* Replaces: cNeuralNet::LoadScale (learning/NeuralNet.cpp:137-215) and cNeuralNet::WriteOffsetScale (:1182-1205): the
 * "<model>_scale.txt" normaliser files ({"InputOffset": [...], "InputScale": [...], "OutputOffset": [...], "OutputScale": [...]},
 * values printed with std::to_string). Loading keeps the weights, replaces the vectors present in the file (absent keys keep their
 * current value, a wrong length is an error, as in the reference); the batch must have been built with -policy_net=. */
dtrl_status dtrl_load_scale_file(dtrl_batch* b, const char* path);
dtrl_status dtrl_write_scale_file(dtrl_batch* b, const char* path);

/* Replaces: cScenarioExp::EnableExplore / SetExpRate / SetExpTemp / SetExpBaseActionRate (scenarios/ScenarioExp.cpp:161-206). */
dtrl_status dtrl_set_explore(dtrl_batch* b, int enable, double rate, double temp, double base_rate);

/* Replaces: cScenarioSimChar::SetTerrainParamsLerp (scenarios/ScenarioSimChar.cpp:255-272). */
dtrl_status dtrl_set_terrain_lerp(dtrl_batch* b, double lerp);

/* Replaces: cScenarioExp::IsTupleBufferFull/GetTuples/ResetTupleBuffer (scenarios/ScenarioExp.h:16-38) for the whole batch.
 * rows: [cap][1 + 2S + A] float32 in the MACE replay row layout [r | s | a | s'] (learning/MACETrainer.cpp:373-401).
 * Where the rings live is a creation argument: `-tuple_ring= device` (default; the drain is a count read-back plus three copies through a page-locked staging
 * area, two synchronisations) or `-tuple_ring= host` (page-locked host memory the kernels write directly: the drain queues NOTHING on the GPU -- with frames
 * in flight every queued copy can wait milliseconds for a wavefront slot, measured 1.2-2.3 ms for the 4-byte count alone). Same rows either way. */
dtrl_status dtrl_drain_tuples(dtrl_batch* b, float* rows, uint32_t* flags, int32_t* env_ids, int cap, int* out_n);

/* dtrl_drain_tuples with DEVICE destination buffers (e.g. the trainer's replay tensors on the same GPU, or the send buffer of the RCCL tuple
 * gather): device-to-device copies on the batch's stream, completed on return; no host staging. The reference hands tuples to the trainer by
 * reference under its lock (learning/NeuralNetLearner.cpp:33-46). flags_dev / env_ids_dev may be NULL. */
dtrl_status dtrl_drain_tuples_device(dtrl_batch* b, float* rows_dev, uint32_t* flags_dev, int32_t* env_ids_dev, int cap, int* out_n);
/* Replaces: the same three calls as dtrl_drain_tuples_device, plus the per-rank packing the reference's learner thread does before it hands tuples to
 * the trainer (learning/NeuralNetLearner.cpp:33-46) -- for a consumer that wants ONE device block it can put on the wire as it is (one RCCL
 * gather per frame). block_dev: [block_rows + 1][W + 2] float32 in DEVICE memory. Row 0 is a header (int32 bit patterns: [0] = number of rows that
 * follow, [1] = rows lost because the RING was full since the last drain -- counted in dtrl_tuple_stats --, [2] = rows carried); rows 1..n are the
 * pending tuples sorted by env id (stable: an env's tuples stay in time order), each [r | s | a | s' | flag word | GLOBAL env id], the last two as int32
 * bit patterns. Rows that do not fit block_rows are CARRIED, not dropped: they move to the front of the ring, in order, and the next drain of that ring
 * hands them out in front of the newer rows -- so a consumer can size its block for the steady state (~0.08 rows per env and frame) instead of for the
 * worst case. Everything runs on the device (segmented counting sort by env id, copy and header kernels); out_n, when not NULL, costs one 4-byte read-back. */
dtrl_status dtrl_drain_tuples_packed(dtrl_batch* b, float* block_dev, int block_rows, int* out_n);
/* Replaces: the concurrency of the reference's learner threads -- an env thread hands its tuples to the trainer under the trainer's lock while the other
 * env threads keep stepping (scenarios/ScenarioTrain.cpp:322-338, 376-410; learning/NeuralNetLearner.cpp:33-46). Batched equivalent: with pipelining on,
 * every dtrl_step_begin switches between two tuple rings, and a drain issued between dtrl_step_begin(f + 1) and dtrl_step_end(f + 1) returns the tuples of
 * frame f from the ring that frame wrote, on a stream of its own, without waiting for frame f + 1 (dtrl_step_end(f); dtrl_step_begin(f + 1);
 * dtrl_drain_tuples_packed(...) -> frame f's tuples while f + 1 runs). Outside a pending step a drain returns the ring of the last frame, as without
 * pipelining. Off by default; the caller drains every frame while it is on (an undrained ring is not lost: it is appended to two frames later). Switching it off
 * requires the idle ring to be empty. */
dtrl_status dtrl_set_tuple_pipelining(dtrl_batch* b, int on);
/* dtrl_step_end followed by dtrl_step_begin(dt) without the barrier between them (same results): each env group receives its frame-boundary host
 * work and its next launch as soon as its own frame is done, so the slowest wavefronts of one group are covered by the other groups' next launches --
 * what dtrl_run_frames does inside, one frame at a time, for callers that act between frames (drain tuples, scenarios/ScenarioTrain.cpp:376-410).
 * Without a pending step it is dtrl_step_begin. */
dtrl_status dtrl_step_end_begin(dtrl_batch* b, double dt);
/* For a caller that works for milliseconds between two dtrl_step_end_begin calls (a trainer going through the drained tuples, one Train() per 32 of them --
 * the reference's env threads keep stepping meanwhile, scenarios/ScenarioTrain.cpp:376-410). Never blocks: every env group whose frame has ALREADY ended gets its
 * frame-boundary work and its next launch now (writing the ring the caller has just drained) instead of waiting for the caller to come back; *relaunched (may be
 * NULL) = how many groups that was. The next dtrl_step_end_begin then handles the other groups only. Needs tuple pipelining, `-tuple_ring= host` (the idle ring's
 * cursor is checked without queueing a copy) and host terrain mode; otherwise, or when the idle ring still holds rows, it does nothing. After a relaunch both rings
 * are being written: tuple drains and dtrl_step_end are refused until the next dtrl_step_end_begin. A group relaunched here runs its frame with the policy of the
 * last hand-over that had taken effect (one frame staler than the groups relaunched later). */
dtrl_status dtrl_step_poll(dtrl_batch* b, double dt, int* relaunched);
/* The reference never drops a tuple (scenarios/ScenarioTrain.cpp:376-410 trains whenever a scene's buffer is full). Here the ring holds
 * max(2 num_envs, -tuple_buffer_size=) rows (-tuple_ring_capacity= overrides); rows completed while it is full are COUNTED, not stored:
 * pending = rows waiting in the ring, drained = rows handed out so far, dropped = rows lost to a full ring since creation (stays 0 when
 * the caller drains at least every ~2 gait cycles), capacity = ring size. Any output may be NULL. */
dtrl_status dtrl_tuple_stats(dtrl_batch* b, int64_t* pending, int64_t* drained, int64_t* dropped, int32_t* capacity);
/* dtrl_set_policy with every pointer in DEVICE memory (cNeuralNet::CopyModel is a memcpy per blob between two nets of one process,
 * learning/NeuralNet.cpp:636-658): the trainer's weight blob -- same Caffe blob order -- is re-laid into the kernel's layout by a gather kernel;
 * NULL normaliser pointers keep the current vectors. Between dtrl_step_begin and dtrl_step_end a weights-only call does not wait for the frame in flight: the
 * weights are gathered into a second buffer (weights_dev may be changed when the call returns) and every env's NEXT frame launch runs with them -- the moment the
 * waiting form takes effect, too. */
dtrl_status dtrl_set_policy_device(dtrl_batch* b, const float* weights_dev, size_t n, const double* in_off_dev, const double* in_scale_dev, const double* out_off_dev, const double* out_scale_dev);
/* The weights-only form with the re-layout kernel queued on a stream of the CALLER's (a hipStream_t; the trainer's): it follows whatever the caller has queued
 * there -- the trainer's last step -- and the call returns when it has run, so ONE host wait covers the trainer's pending work and the hand-over (during a frame the
 * engine's own stream would have to find a wavefront slot of its own). Same semantics as dtrl_set_policy_device otherwise. */
dtrl_status dtrl_set_policy_device_on(dtrl_batch* b, const float* weights_dev, size_t n, void* stream);
/* The weights-only form with NO host wait: the re-layout kernel is queued on `stream` (a hipStream_t of the caller's, required) behind whatever produced
 * weights_dev there -- an RCCL broadcast of cNeuralNetLearner::SyncNet's payload (learning/NeuralNetLearner.cpp:85-89), the trainer's last step -- and every env's
 * NEXT frame launch waits for it ON THE DEVICE and runs with the new weights. Valid with or without a frame in flight. weights_dev must not change until the
 * work queued on `stream` has passed this point (the caller's next write to it on the same stream is ordered by the stream). Needs normalisers installed by an
 * earlier dtrl_set_policy / dtrl_set_policy_device. */
dtrl_status dtrl_set_policy_device_async(dtrl_batch* b, const float* weights_dev, size_t n, void* stream);

/* No counterpart in the reference (its trainer and its env threads share CPU cores under the OS scheduler; scenarios/ScenarioTrain.cpp runs them as threads
 * of one process). On the GPU a frame launch fills every wavefront slot of the compute units it may use for milliseconds, so work that should run BESIDE the
 * rollout -- the trainer's kernels, the exchange's collective -- needs (1) compute units the frame launches leave alone: `-reserve_cus= k` at creation (or
 * DTRL_RESERVE_CUS=k) keeps k units per XCD out of them (k / 32 of the rollout rate), and (2) a hardware queue that is not held up by a frame launch waiting
 * for slots: the engine measures its candidate streams at creation and hands out the two quickest. Returns a hipStream_t (k = 0, 1) owned by the batch, or
 * NULL without a reservation; *start_delay_us (may be NULL) = how long a burst of 10 small kernels on that stream took beside two frame-sized occupant
 * launches during the calibration (microseconds: about 70 on a free queue, a thousand or more on a held-up one). */
void* dtrl_side_stream(dtrl_batch* b, int k, double* start_delay_us);

/* Replaces: cSimCharacter::BuildPose / BuildVel (sim/SimCharacter.cpp:166-225). env_ids == NULL -> envs 0..n-1. */
dtrl_status dtrl_get_pose_vel(dtrl_batch* b, const int32_t* env_ids, int n, double* q, double* qd);
/* Replaces: cCharController::CommandAction (sim/CharController.h:23, sim/DogController.cpp:309-320): action_ids[i] (an index into the controller's
 * action table, dtrl_get_action_table) is the base action env i takes at its next cycle instead of asking the policy. env_ids == NULL -> envs 0..n-1 =
 * all envs, action_ids then holds num_envs entries. The reference keeps a stack of commands; the engine keeps its top only (one pending command per env,
 * a new one replaces it -- also the random first action cScenarioExp::Reset queues, scenarios/ScenarioExp.cpp:63-73). */
dtrl_status dtrl_command_action(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* action_ids);
/* Replaces: cSimCharacter::SetPose / SetVel (sim/SimCharacter.cpp:665-683, 227-315). A teleported character drops its persistent contact rows (what Bullet's
 * refreshContactPoints does to manifold points that moved out of the breaking threshold): restoring a saved state = dtrl_set_pose_vel, THEN dtrl_set_contact_cache. */
dtrl_status dtrl_set_pose_vel(dtrl_batch* b, const int32_t* env_ids, int n, const double* q, const double* qd);
/* Replaces: the state Bullet's collision world keeps BETWEEN stepSimulation calls besides the bodies' poses and velocities: the persistent contact points of
 * the dispatcher's manifolds with their applied normal / friction impulses (btManifoldPoint::m_appliedImpulse, m_appliedImpulseLateral1), which the default
 * btSequentialImpulseConstraintSolver the reference builds (sim/World.cpp:61-77) warm-starts from with factor 0.85. A character's dynamic state is (q, qd) PLUS this
 * cache: whoever saves, restores or transplants a character mid-run (checkpointing, the side-by-side parity tests) moves both. Per env i: count[i] rows
 * (<= DTRL_MAX_CONTACT_ROWS), ids[i][k] = identity of row k (ground contact 2 x sample point + (0 normal, 1 tangent); link--link contact 512 + 2 x (pair x 12 +
 * candidate) + (0, 1); 65535 = a joint-limit row, never matched) and lambda[i][k] = the impulse it ended the last substep with. cWorld::Reset empties it. */
#define DTRL_MAX_CONTACT_ROWS 24
dtrl_status dtrl_get_contact_cache(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* count, int32_t* ids, double* lambda);
dtrl_status dtrl_set_contact_cache(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* count, const int32_t* ids, const double* lambda);

/* ---- full env snapshots: save, restore, clone, export ----
 * No counterpart in the reference: it keeps ONE scene per object (a cScenarioSimChar owns its world, character, controller and ground; the learner threads of
 * scenarios/ScenarioTrain.cpp:100-115 own one each) and never copies a running scene. A batch of thousands of envs needs what a rollout engine's users expect:
 * checkpoint the envs of a long run, rewind a batch and try something else, duplicate an interesting env, hand a full state to another process.
 * dtrl_set_pose_vel + dtrl_set_contact_cache move the Bullet half of an env only. A SNAPSHOT is an object owned by the library that holds, for a list of envs of
 * one batch, everything that decides their future, with its payload in DEVICE memory (saving and restoring is one kernel launch, no host round trip per env):
 *   - the whole env state record: pose, velocity, torques, the persistent contact rows; FSM state, phase, current action id and parameters, PD targets, cycle
 *     timers and stumble times (the members of sim/DogController.cpp:805-845 and sim/RaptorController.cpp:804-849 -- mState, mPhase, mCurrAction, mCurrCycleTime,
 *     mPrevCycleTime, mPrevStumbleCount, mCurrStumbleCount ..., stance leg and PD active flags of the raptor); the soft-fall filter and its counters
 *     (sim/SimCharSoftFall.cpp:74-125: mFallDistCounter, mFallContactCounter, mSumFallContact, the previous check position); distance and episode bookkeeping, the
 *     exploration counter, a pending commanded action, the perturbation slot, and the pending reset / init flags (a snapshot taken after a fall and before
 *     the env's next launch replays that reset);
 *   - the ground: the two-segment window the kernels sample (cGroundVar2D's mSegments, sim/GroundVar2D.cpp) and what decides the segments built AFTER a restore --
 *     the host generator's window with both segments, mFlipSeg, its build count and its cRand state, or with `-terrain_gen= device` the env's generator counters;
 *     a regenerated window still waiting for the env's next launch is the one saved, and a restore supersedes a waiting one;
 *   - the policy state recorded for the current action, the begin state and action of the tuple in progress (anim/Character.cpp:217-262 is what the reference
 *     could write out -- a pose and a velocity; cScenarioExp's mCurrTuple has no writer at all) and the net's last output;
 *   - the env's status record (root x, which drives the window slide; the launch-order cost; a pending reset request).
 * A snapshot does NOT hold what belongs to the batch or is an output of it: policy weights and normalisers, the exploration settings (dtrl_set_explore), the
 * terrain lerp, a policy hand-over still pending, the tuple rings with their drained / dropped totals, and the dist log.
 * Exploration streams are keyed by (seed, GLOBAL env id, per-env counter): an env restored into its own slot continues bit-identically; an env transplanted or
 * cloned into another slot carries its counter along and continues with THAT slot's stream.
 * None of these calls waits for a frame in flight: between dtrl_step_begin and dtrl_step_end (or after dtrl_step_poll relaunched a group) save, restore,
 * clone, export and import fail with DTRL_ERR_ARG. Env ids out of range, and a slot listed twice as a destination, are DTRL_ERR_ARG. */
typedef struct dtrl_snapshot dtrl_snapshot;
/* Save the listed envs (env_ids == NULL: all, n ignored) into a new snapshot; the slot list is kept in it. Free it with dtrl_snapshot_free. */
dtrl_status dtrl_snapshot_save(dtrl_batch* b, const int32_t* env_ids, int n, dtrl_snapshot** out);
/* env_ids == NULL: every saved env goes back into the slot it came from. Otherwise the first n saved envs, in saved order, go into the listed slots (a saved env
 * transplanted into another slot). The snapshot must have been saved by, or imported into, this batch; it is compared with the batch like a blob (below). */
dtrl_status dtrl_snapshot_restore(dtrl_batch* b, const dtrl_snapshot* snap, const int32_t* env_ids, int n);
/* Env dst_ids[i] becomes a copy of env src_ids[i], inside one batch, without a snapshot object. A source may repeat; destinations are distinct. Lists that
 * overlap behave as "read all, then write all" (src = {0, 1}, dst = {1, 2}: env 2 gets the OLD env 1). */
dtrl_status dtrl_clone_envs(dtrl_batch* b, const int32_t* src_ids, const int32_t* dst_ids, int n);
/* One flat, self-describing host blob: a header (magic "DTRLSNP1", format version, sizeof(real), sizeof(EnvState), sizeof(GroundRec) and the other record sizes,
 * character and controller type, L, D, S, A, the net's output size, the terrain mode, bytes per env, env count, the policy mode), the saved slot ids, the device payload
 * [n][bytes per env] (each env: EnvState first, then GroundRec, ...), the host payload. *bytes = the blob's size; cap == 0 returns the size only; a smaller
 * buffer is DTRL_ERR_CAPACITY. Needs the batch that holds the snapshot to be alive and idle (errors are reported through that batch's dtrl_last_error). */
dtrl_status dtrl_snapshot_export(const dtrl_snapshot* snap, void* buf, size_t cap, size_t* bytes);
/* A blob -> a snapshot held by batch b. The header is compared with the batch, field by field: another character or controller, the other precision's library
 * (sizeof(real)), another terrain mode, other sizes, a wrong magic or version, a truncated blob are refused with DTRL_ERR_ARG and a message naming the field.
 * The values the kernels use as indices (action ids, row counts, segment widths ...) are range-checked, so that an edited blob cannot address out of bounds. */
dtrl_status dtrl_snapshot_import(dtrl_batch* b, const void* blob, size_t bytes, dtrl_snapshot** out);
/* Any output may be NULL: number of envs, device payload bytes per env, sizeof(EnvState) of the library that made it (the record at the start of every env's
 * payload slice, dtrl_types.h), host payload bytes per env. */
dtrl_status dtrl_snapshot_info(const dtrl_snapshot* snap, int32_t* n_envs, size_t* bytes_per_env, size_t* sizeof_env_state, size_t* host_bytes_per_env);
/* Valid before or after dtrl_destroy of the batch (which releases the payload; the handle then only answers dtrl_snapshot_info). */
dtrl_status dtrl_snapshot_free(dtrl_snapshot* snap);

/* ---- External policy mode: the caller's policy in place of the net inside the frame kernel (`-policy_mode= external`; default `internal`) ----
 * Replaces: the decision inside cBaseControllerMACE::UpdateAction -- DecideAction / DecideActionBoltzmann and the forward behind it
 * (sim/BaseControllerMACE.cpp:267-296) -- through the seam the reference itself has: a controller takes a commanded action from outside
 * (cCharController::CommandAction, sim/CharController.h:23) and cScenarioExp hands every decision's state and action to a learner it does not own
 * (scenarios/ScenarioExp.cpp:63-73). MACE controllers only (dog_mace, goat_mace, raptor_mace): with a Q or CACLA controller dtrl_create fails with DTRL_ERR_ARG.
 *
 * Every env keeps its own frame of num_update_steps env-steps. dtrl_step (or dtrl_step_begin / dtrl_step_end) is a TICK: an env whose frame is complete
 * starts a new one; every env runs until its frame is complete (falls, resets and episode bookkeeping happen there, as in internal mode) or until its gait
 * cycle ends and it needs an action, whichever comes first. An env that needs an action PARKS behind the physics of that env-step, with its policy state
 * built (ParseGround / BuildPoliState); a pending commanded action -- dtrl_command_action, the random first action of an Exp episode -- is served without
 * asking. A parked env that has been given its action finishes that env-step and the rest of its frame in the next tick; one that has not stays exactly as
 * it is. The env-steps, decisions and fall checks of one env are the sequence internal mode runs; only their grouping into launches differs. Terrain windows,
 * resets and the dist log are handled in the tick in which an env completes its frame.
 *
 * An action row is what the MACE branch would have produced: action_id (a label, 0 .. number of base actions - 1: stored as the current action id and in the
 * tuple), params[frag_size of dtrl_action_dims] (written over the current parameters at the optimisable indices, then PostProcessParams and ApplyAction), and
 * an optional flag word in the tuple-flag layout (DTRL_TUPLE_EXP_CRITIC, DTRL_TUPLE_EXP_ACTOR: what the tuple that starts here is recorded with).
 * dtrl_set_explore is ignored at these decisions: the caller explores.
 *
 * Refused in this mode (DTRL_ERR_ARG): dtrl_step_updates, dtrl_run_frames, dtrl_step_poll, dtrl_step_end_begin, dtrl_set_tuple_pipelining(1), dtrl_set_policy*,
 * dtrl_load_scale_file. The calls below fail with DTRL_ERR_ARG on an internal-mode batch, and -- they never wait -- between dtrl_step_begin and dtrl_step_end.
 * Snapshots carry the park state and a delivered action; a blob of one mode is refused by a batch of the other. */
/* The awaiting envs in ascending env id: env_ids[0 .. *out_n) and their policy states states[*out_n][S of dtrl_dims] (may be NULL); at most cap of them. */
dtrl_status dtrl_pending_actions(dtrl_batch* b, int32_t* env_ids, double* states, int cap, int* out_n);
/* The same into DEVICE memory, states as float (a torch policy on the same GPU reads them in place). The arrays are complete when the call returns. */
dtrl_status dtrl_pending_actions_device(dtrl_batch* b, int32_t* env_ids_dev, float* states_dev, int cap, int* out_n);
/* n rows (host memory) for n distinct awaiting envs; action_ids and flags may be NULL (zeros). All or nothing: an id that is out of range, named twice or not
 * awaiting, or a label out of range, is DTRL_ERR_ARG and nothing is applied. */
dtrl_status dtrl_supply_actions(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* action_ids, const double* params, const uint32_t* flags);
/* n rows in DEVICE memory (params as float; the caller's stream must have finished writing them). A row that does not apply -- id or label out of range, env
 * not awaiting, env named by an earlier row -- is skipped, changes nothing and is counted in *rejected (may be NULL); the call still returns DTRL_OK. */
dtrl_status dtrl_supply_actions_device(dtrl_batch* b, const int32_t* env_ids_dev, int n, const int32_t* action_ids_dev, const float* params_dev, const uint32_t* flags_dev, int* rejected);
/* Envs parked without / with a delivered action now; env-steps run and env frames completed by all envs since creation (counted on the device per env,
 * what a throughput figure in this mode has to be taken from: a tick advances an env by anything between 0 and num_update_steps env-steps). Any may be NULL. */
dtrl_status dtrl_ext_stats(dtrl_batch* b, int64_t* awaiting, int64_t* ready, int64_t* env_steps_total, int64_t* env_frames_total);
/* Per env: park state (0 running / frame complete, 1 awaiting, 2 action delivered) and the env-steps its current frame still has to finish (0: complete). */
dtrl_status dtrl_ext_env_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* park, int32_t* steps_left);
/* What an action row is made of: n_opt = params per row (cTerrainRLCharController::GetNumOptParams), n_labels = valid action_id values 0 .. n_labels - 1,
 * num_update_steps = env-steps per env frame, external = 1 for a -policy_mode= external batch. Works in either mode; any output may be NULL. */
dtrl_status dtrl_action_dims(const dtrl_batch* b, int* n_opt, int* n_labels, int* num_update_steps, int* external);
/* Device time (ms, HIP events) of the collection (which = 0) / scatter (which = 1) launches since the previous call; -1 where nothing is launched. */
double dtrl_ext_launch_ms(dtrl_batch* b, int which);

/* ---- Policy slots: several policies in one batch, one per env ----
 * No counterpart in the reference: it keeps one net per scene object (the controller's cNeuralNet, sim/NNController.cpp:49-78), so comparing or mixing
 * policies there means one scenario per policy. A slot is a set of weights, the four normalisers and the exploration settings; a batch holds up to 32 and every
 * env is assigned to one. Frames still run as one launch per env group. Slot 0 IS the batch's policy: dtrl_set_policy*, dtrl_load_scale_file and dtrl_set_explore
 * keep acting on it (double-buffered and asynchronous hand-overs included), and every env starts in it. Every other slot starts without a policy and with the
 * exploration settings the batch has at dtrl_slots_create. A batch that never calls dtrl_slots_create runs exactly
 * the kernels and launches it ran before. `exp_noise` stays the batch's. The assignment is batch state like the policy: snapshots, restores, clones and blobs do
 * not carry it and a reset does not change it. Slots use local env ids (a sharded run has slots per shard). Not available in external policy mode.
 * Except where noted the calls below are refused with DTRL_ERR_ARG between dtrl_step_begin and dtrl_step_end (they never wait for a frame), and then wait for
 * everything the batch has queued on the device before they change anything: no launch ever sees a half-written slot. */
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). 1 <= n_slots <= 32, once per batch (the same count again is
 * accepted). Refused with DTRL_ERR_ARG: external policy mode, a batch without -policy_net=, a frame in flight, a second call with another count. */
dtrl_status dtrl_slots_create(dtrl_batch* b, int n_slots);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). dtrl_set_policy into a slot: the same blob order and
 * relayout, NULL normalisers mean identity. Slot >= 1 gets weight and normaliser storage of its own on first use and stops being an alias; slot 0 is
 * dtrl_set_policy itself. Synchronous. */
dtrl_status dtrl_slot_set_policy(dtrl_batch* b, int slot, const float* weights, size_t n, const double* in_off, const double* in_scale, const double* out_off, const double* out_scale);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). The same from DEVICE memory (dtrl_set_policy_device's
 * conventions: a NULL normaliser keeps the slot's current vector, identity in a slot that had no policy yet; the fp32 library takes weights only). Synchronous. */
dtrl_status dtrl_slot_set_policy_device(dtrl_batch* b, int slot, const float* weights_dev, size_t n, const double* in_off_dev, const double* in_scale_dev, const double* out_off_dev, const double* out_scale_dev);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). Slot (>= 1) reads src_slot's weights and normalisers from now
 * on, whatever they become -- every hand-over into slot 0 included -- and keeps exploration settings of its own: "the same net, greedy" at no memory cost.
 * Refused: an alias of itself (directly or through other aliases), an empty source slot. */
dtrl_status dtrl_slot_alias(dtrl_batch* b, int slot, int src_slot);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). dtrl_set_explore for one slot; slot 0 is dtrl_set_explore
 * itself (and, like it, valid at any time). */
dtrl_status dtrl_slot_set_explore(dtrl_batch* b, int slot, int enable, double rate, double temp, double base_rate);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). env_ids[i] -> slots[i]; env_ids == NULL means the first n
 * envs. All or nothing: an env id or slot out of range, or a slot that has neither a policy nor an alias, is DTRL_ERR_ARG. Takes effect with the env's next
 * launch: a mid-cycle env makes its next decision with the new slot, nothing else in its state changes. */
dtrl_status dtrl_assign_slots(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* slots);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). The slots of the listed envs (valid at any time). With the
 * env id column of dtrl_drain_tuples this tells which slot produced a tuple. */
dtrl_status dtrl_get_slots(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* slots_out);
/* No counterpart in the reference: it keeps one net per scene object (sim/NNController.cpp:49-78). dtrl_eval_stats restricted to the envs currently in the slot
 * (n_envs of them), reduced on the device in a fixed order: two calls without a step between them return the same bits. Any output may be NULL. */
dtrl_status dtrl_slot_stats(dtrl_batch* b, int slot, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);

/* ---- Model variants: several character models in one batch, one per env ----
 * No counterpart in the reference, which keeps one character per scene object (cScenarioSimChar::BuildCharacter, scenarios/ScenarioSimChar.cpp): training or
 * measuring a policy across masses, sizes or motor strengths there means one scenario per model. A variant is a complete character model (masses, inertias,
 * box sizes, attach points, joint limits, PD gains, torque limits and every table derived from them); a batch holds a table of n_variants of them, up to one per
 * env, and a per-env index says which one an env runs. The table costs sizeof(DevModel) per variant in device memory: 14 352 bytes in the fp64 library, 8 276 in
 * the fp32 library. Frames still run as one launch per env group. Variant 0 IS the batch's own model; every env starts in it; variants >= 1 start empty. A batch
 * that never calls dtrl_variants_create runs exactly the kernels and launches it ran before. The assignment is batch state like the slot assignment: snapshots,
 * restores, clones and blobs do not carry it and a reset does not change it. An env that changes variant keeps every byte of its state and simply runs its next
 * launch under the other model; a caller who wants episodes to START under the new model resets those envs (dtrl_reset) after assigning. Variants use local
 * env ids. Not available together with policy slots or with -policy_mode= external, in either order (each combination would be one more kernel family);
 * terrain sets (below) combine with all three.
 * The calls below are refused with DTRL_ERR_ARG between dtrl_step_begin and dtrl_step_end (they never wait for a frame) and then -- dtrl_get_variants
 * excepted, which is valid at any time -- wait for everything the batch has queued on the device before they change or read anything. */
/* No counterpart in the reference, which keeps one character per scene object. 1 <= n_variants <= num_envs, once per batch, between frames. Refused with
 * DTRL_ERR_ARG: a second call, a batch with policy slots, external policy mode, a frame in flight. */
dtrl_status dtrl_variants_create(dtrl_batch* b, int n_variants);
/* No counterpart in the reference, which keeps one character per scene object. Fill variant v >= 1 from a character file: the loader the batch was created
 * with runs again on the creation arguments with only the character description replaced, so every derived table comes out of the one code path. The path is
 * resolved like -character_file= (relative to -data_root=, absolute paths as they are). DTRL_ERR_ARG, naming the field, when the variant does not fit the
 * batch: the skeleton (L, D, parent), the scene (char_type, ctrl_type, scenario, num_update_steps, num_sim_substeps, world_scale, valid_init_pos_x) and the whole
 * controller part (P, n_opt, opt_index, n_sets, ctrl_params, n_actions, the action tables, default_action, enable_grav_comp, enable_vf) must equal variant 0:
 * the batch has one policy, one action table and one set of output normalisers. Everything else may differ. DTRL_ERR_IO: the file cannot be read or parsed. */
dtrl_status dtrl_variant_load_file(dtrl_batch* b, int v, const char* character_file);
/* No counterpart in the reference, which keeps one character per scene object. The same from `bytes` bytes of JSON text in memory (a character file's content). */
dtrl_status dtrl_variant_load_json(dtrl_batch* b, int v, const char* text, size_t bytes);
/* No counterpart in the reference, which keeps one character per scene object. env_ids[i] -> variants[i]; env_ids == NULL means the first n envs (n = num_envs:
 * all). All or nothing: an env id or variant out of range, or an empty variant, is DTRL_ERR_ARG. Takes effect with the env's next launch. */
dtrl_status dtrl_assign_variants(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* variants);
/* No counterpart in the reference, which keeps one character per scene object. The variants of the listed envs. Without a variant redraw (below), and with one
 * in host terrain mode: valid at any time. With a redraw and -terrain_gen= device the variants move on the device at the frame boundaries: the call then returns
 * them as of the last completed boundary -- it is refused with DTRL_ERR_ARG between dtrl_step_begin and dtrl_step_end, and otherwise waits for everything the
 * batch has queued. */
dtrl_status dtrl_get_variants(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* variants_out);
/* No counterpart in the reference, which keeps one character per scene object. dtrl_eval_stats restricted to the envs currently in variant v (n_envs of them),
 * reduced on the device in a fixed order: two calls without a step between them return the same bits. Any output may be NULL. */
dtrl_status dtrl_variant_stats(dtrl_batch* b, int v, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);

/* ---- Variant redraw: envs draw a new model variant at each episode start (domain randomisation while training) ----
 * No counterpart in the reference, which keeps one character per scene object. A redraw is a contiguous range [lo, hi] of filled variants, a seed and a weight per
 * variant of the range. Each env carries a counter `draws`. At env e's EPISODE START -- a frame boundary at which it fell (need_reset bit 0), or dtrl_reset naming
 * it (once per env, however often it is listed) -- with k = the env's variant:
 *   k outside [lo, hi]      nothing: the env is not in the redraw (evaluation envs can be held on variant 0 that way)
 *   else                    bits = mix(mix(mix(seed) ^ (C + global env id)) + draws * 0xD1342543DE82EF95), u = (bits >> 11) * 2^-53,
 *                           k = lo + #{ j : cum[j] <= u } (clamped to hi), draws += 1
 * mix is the terrain streams' 64-bit finaliser and C a constant of the redraw's own; cum[j] = (w_0 + .. + w_j) / (w_0 + .. + w_(hi-lo)), summed left to right
 * in double, the last entry exactly 1.0 (uniform: every w_j = 1). The draw is a function of the seed, the GLOBAL env id (-env_id_base= + local id) and the
 * env's own counter alone: shard-invariant, and independent of exploration, reward and every other env. The rule runs IN FRONT OF the reset launch, so the
 * device half of the reset (default pose, centre of mass, forward kinematics) is the new variant's; the frame that ended, with its fall bookkeeping, ran under
 * the old one. dtrl_assign_terrains with restart != 0 does not draw. With -terrain_gen= device the rule is one more small launch per env group and frame,
 * queued with the boundary work (no host round trip; dtrl_run_frames and the overlapped loops included); in host terrain mode it runs in the host's per-frame
 * status loop. Settings and counters are batch state like the assignment: snapshots, restores, clones and blobs leave them alone. Internal policy mode only, as
 * the variants themselves. */
/* No counterpart in the reference, which keeps one character per scene object. Turn the redraw on (lo <= hi), replace its settings, or remove it (lo > hi; the
 * envs keep the variants they have). The counters are kept in all three cases. weights: NULL = uniform over lo..hi, else hi - lo + 1 non-negative finite doubles,
 * not all zero. DTRL_ERR_ARG, nothing changed: no variants, lo / hi outside the table, an empty variant inside [lo, hi], a negative, NaN or infinite weight, all
 * weights zero, a frame in flight. */
dtrl_status dtrl_variant_redraw(dtrl_batch* b, int lo, int hi, uint64_t seed, const double* weights);
/* No counterpart in the reference, which keeps one character per scene object. Any output may be NULL. The redraw's range, and per listed env (env_ids == NULL:
 * the first n) its variant now and how many draws it has made, as of the last completed boundary: refused between dtrl_step_begin and dtrl_step_end and without
 * a redraw, otherwise waits for queued work. */
dtrl_status dtrl_variant_redraw_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* lo, int32_t* hi, int32_t* variant, int32_t* draws);

/* ---- Variant rescale: per-episode continuous mass and motor scales, drawn on the device ----
 * No counterpart in the reference, which keeps one character per scene object. Where the redraw picks among the table's models, the rescale gives an env a PRIVATE
 * model record and rewrites its mass and motor scalars from ranges at every episode start. With V = n_variants, the first call grows the device table once to
 * V + num_envs records (with the streams idle, the old records copied): sizeof(DevModel) more per env -- 14 352 bytes in the fp64 library, 8 276 in the fp32
 * library; 59 MB at 4096 envs in fp64. An env e that joins gets key V + e; its private record starts as a copy of variant `base` (all factors 1). At env e's
 * EPISODE START -- a frame boundary at which it fell (need_reset bit 0), or dtrl_reset naming it -- while its key is V + e, with n = the env's `episodes`:
 *   key    = mix(mix(seed) ^ (C + global env id))                                   (mix: the terrain streams' 64-bit finaliser, C a constant of the rescale's own)
 *   u(q,j) = (mix(key + (n * 4 * L + q * L + j) * 0xD1342543DE82EF95) >> 11) * 2^-53   q = 0 mass, 1 kp, 2 kd, 3 torque_lim
 *   f_q[j] = lo_q + u(q, j') * (hi_q - lo_q),  j' = j when bit q of per_link is set (one factor per link), else 0 (one factor for all links)
 *   mass[j] = m0[j] * f_0[j]; total_mass, inertia[j] = mass[j] / 12 * (sx^2 + sy^2) and the subtree masses follow; kp, kd, torque_lim[j] = base value * f[j]
 *   episodes += 1
 * The base values are the character file's doubles, every product is taken in double and cast once, and every derived field is computed by the loader's
 * formulas in the loader's order: the record holds the bits dtrl_variant_load_json would load from the base's character file with Mass, Kp, Kd and TorqueLim
 * multiplied by the same factors -- in the fp32 library too. The index layout is fixed, so switching a quantity between uniform and per-link moves no other
 * quantity's draws. The draw is a function of the seed, the GLOBAL env id and the env's episode number alone: shard-invariant, independent of exploration and
 * of every other env. Only these scalars move: geometry, margins, contact points and limits are the base's (size scaling would move them and stays a matter of
 * the table: ScaledVariant). The rule is one small launch per env group and frame in BOTH terrain modes, queued on the group's stream behind the variant redraw
 * and in front of the push schedule and the reset launch, which therefore runs under the new scales; no host wait is added. Nothing else writes a record while
 * launches run. Keys >= V appear in dtrl_get_variants; dtrl_assign_variants does not accept them (its range check stays), and assigning an ordinary variant to
 * an env takes it out of the rescale. The redraw acts on keys below V only, so both rules can be on. dtrl_variant_stats keeps its range 0 .. V - 1.
 * dtrl_get_link_states and dtrl_add_perturb read the base's geometry for an env under a private key. Settings, counters and private records are batch state
 * like the assignment: snapshots, restores, clones and blobs leave them alone. */
/* The four ranges {lo, hi} (0 < lo <= hi, finite; {1, 1} = not scaled) and the per_link mask (bit 0 mass, 1 kp, 2 kd, 3 torque_lim). */
typedef struct dtrl_rescale_desc { double mass[2], kp[2], kd[2], torque_lim[2]; uint32_t per_link; uint32_t reserved; } dtrl_rescale_desc;
/* No counterpart in the reference, which keeps one character per scene object. Turn the rescale on or replace its settings (desc != NULL), and put the listed
 * envs under their private records (env_ids == NULL: the first n envs, n = num_envs: all; n = 0: the settings only). desc == NULL removes the rescale: its envs
 * go back to key `base` of the rescale, the counters are kept. DTRL_ERR_ARG, nothing changed: no variants, base out of range or empty, a range with lo <= 0,
 * lo > hi or a NaN or infinite bound, per_link bits beyond the four, an env id out of range, another base than the rescale's while envs run under private
 * records, a frame in flight. While the rescale is on, dtrl_variant_load_* into its base is refused. */
dtrl_status dtrl_variant_rescale(dtrl_batch* b, int base, const int32_t* env_ids, int n, uint64_t seed, const dtrl_rescale_desc* desc);
/* No counterpart in the reference, which keeps one character per scene object. Any output may be NULL. The rescale's base, seed and settings, and per listed env
 * (env_ids == NULL: the first n) its key, its episode count and the factors [n][4][L] of its CURRENT episode (recomputed on the host by the same rule from
 * episodes - 1; all 1 for an env that is not under its private key or has started no episode yet), as of the last completed boundary: refused between
 * dtrl_step_begin and dtrl_step_end and without a rescale, otherwise waits for queued work. */
dtrl_status dtrl_variant_rescale_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* base, uint64_t* seed, dtrl_rescale_desc* desc, int32_t* key, int32_t* episodes, double* factors);
/* No counterpart in the reference, which keeps one character per scene object. The mass and motor scalars of the model record env `env` runs under, read from the
 * DEVICE table (private key or not; a batch without variants: its own model): out[6][L] = mass, inertia, sub_mass, kp, kd, torque_lim as doubles (exact casts of
 * the record's `real`), and total_mass. Either output may be NULL. Refuses a frame in flight and waits for queued work. */
dtrl_status dtrl_variant_scalars(dtrl_batch* b, int env, double* out, double* total_mass);

/* ---- Terrain sets: several terrains in one batch, one per env ----
 * No counterpart in the reference, which keeps one terrain per scene object (cScenarioSimChar::ParseTerrainParams reads ONE -terrain_file= into the scene's
 * cGroundVar2D, scenarios/ScenarioSimChar.cpp:670-706): measuring a policy on flat / slopes_mixed / narrow_gaps / cliffs there means one scenario per terrain, and
 * neither a mixture of terrains nor a per-env curriculum can be expressed. A terrain is the type plus the 40 parameters of cTerrainGen2D::eParams; the scene
 * constants (world scale, segment width, view and spawn bounds) stay the batch's. A batch holds a table of n_terrains of them, up to one per env, and a per-env
 * index says which terrain builds an env's NEXT segments. Terrain 0 IS the batch's terrain: dtrl_set_terrain_lerp and -terrain_blend= keep acting on it (and
 * on the envs in it alone), every env starts in it; terrains >= 1 start empty. No frame kernel reads terrain parameters (they read the env's ground record), so a
 * batch that never calls dtrl_terrains_create runs exactly the launches it ran before, and terrains combine freely with policy slots, model variants and
 * -policy_mode= external, in either order of creation. The assignment is batch state like the slot and variant assignments: snapshots, restores, clones, blobs
 * and dtrl_reset neither carry nor change it; a restored window keeps its segments and generator state and builds its next segment under the env's current
 * terrain. Terrains use local env ids. The calls below are refused with DTRL_ERR_ARG between dtrl_step_begin and dtrl_step_end (they never wait for a frame)
 * and then -- dtrl_get_terrains and dtrl_terrain_info excepted, which are valid at any time -- wait for everything the batch has queued on the device before
 * they change or read anything. */
/* No counterpart in the reference, which keeps one terrain per scene object. 1 <= n_terrains <= num_envs, once per batch (the same count again is accepted), between frames. */
dtrl_status dtrl_terrains_create(dtrl_batch* b, int n_terrains);
/* No counterpart in the reference, which keeps one terrain per scene object. Fill terrain t >= 1 from a terrain file, in place of the file reader of cScenarioSimChar::ParseTerrainParams
 * (scenarios/ScenarioSimChar.cpp:670-706) + cTerrainGen2D::LoadParams (sim/TerrainGen2D.cpp:69-81): the reader creation uses ("Type" plus every 40-vector of
 * "Params", missing values from the defaults), the path resolved like -terrain_file=. `lerp` blends THAT file's parameter sets as dtrl_set_terrain_lerp blends
 * the batch's (scenarios/ScenarioSimChar.cpp:255-272). May be called again for a filled terrain -- that is how a per-terrain curriculum moves: the envs in the
 * terrain build their next segments under the new parameters. DTRL_ERR_IO: the file cannot be read or parsed; DTRL_ERR_ARG: unknown type name, t out of range or 0. */
dtrl_status dtrl_terrain_set_file(dtrl_batch* b, int t, const char* terrain_file, double lerp);
/* No counterpart in the reference, which keeps one terrain per scene object. The same from memory, in place of the file reader (scenarios/ScenarioSimChar.cpp:670-706, sim/TerrainGen2D.cpp:69-81): a type name
 * ("" == flat) and params40 in cTerrainGen2D::eParams order -- what dtrl_terrain_build takes. */
dtrl_status dtrl_terrain_set_params(dtrl_batch* b, int t, const char* type_name, const double* params40);
/* No counterpart in the reference, which keeps one terrain per scene object. What terrain t currently holds: its type name (up to type_cap bytes), its 40 parameters, and whether it has been filled (an empty
 * terrain reports the batch's). For terrain 0: the lerped parameters in force. Any output may be NULL. */
dtrl_status dtrl_terrain_info(dtrl_batch* b, int t, char* type_out, int type_cap, double* params40_out, int* filled_out);
/* No counterpart in the reference, which keeps one terrain per scene object. env_ids[i] -> terrains[i]; env_ids == NULL means the first n envs. All or nothing: an env id or terrain out of range, or an empty
 * terrain, is DTRL_ERR_ARG. restart == 0: takes effect with the env's next segment build -- the window in place stays and the new terrain joins it at the seam
 * height, as a curriculum step does. restart != 0: in the same call the listed envs start over as at creation under their new terrain: the terrain stream is
 * re-seeded from (terrain seed, GLOBAL env id), the build count goes to 0, a fresh two-segment window is built around the spawn point, and the device half of a
 * reset runs (as dtrl_reset). The exploration counter is not rewound. */
dtrl_status dtrl_assign_terrains(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* terrains, int restart);
/* No counterpart in the reference, which keeps one terrain per scene object. The terrains of the listed envs. Without a terrain ladder (below): valid at any time.
 * With a ladder the levels move at the frame boundaries, with -terrain_gen= device on the device: the call then returns the levels as of the last completed
 * boundary -- it is refused with DTRL_ERR_ARG between dtrl_step_begin and dtrl_step_end, and otherwise waits for everything the batch has queued. */
dtrl_status dtrl_get_terrains(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* terrains_out);
/* No counterpart in the reference, which keeps one terrain per scene object. dtrl_eval_stats restricted to the envs currently in terrain t (n_envs of them), reduced on the device in a fixed order: two calls
 * without a step between them return the same bits. Refuses a frame in flight, like dtrl_variant_stats. Any output may be NULL. */
dtrl_status dtrl_terrain_stats(dtrl_batch* b, int t, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);

/* ---- Terrain ladder: envs climb and descend a range of the terrain set by their own episodes ----
 * No counterpart in the reference, which keeps one terrain per scene object and moves it for everybody at once (SetTerrainParamsLerp). A ladder is a contiguous
 * range [lo, hi] of filled terrains, ordered easy to hard by the caller. Each env carries a record {mark_x, ups, downs}: mark_x is the root x at which it last
 * spawned or last changed level. At the frame boundary of env e, IN FRONT OF its terrain work (so the window built or slid in the same boundary is already the
 * new level's), with k = the env's terrain, in double:
 *   k outside [lo, hi]                                    nothing: the env is not on the ladder (evaluation envs can be held on fixed terrains)
 *   the episode ended (the env fell)                      root_x - mark_x < down_dist and k > lo: k -= 1, downs += 1. Always mark_x = spawn_x
 *   it did not, and root_x - mark_x >= up_dist            k < hi: k += 1, ups += 1; else with at_top == 1: k = lo + draw % (hi - lo + 1), ups += 1 (draw: counter-
 *                                                         based, a function of the terrain seed, the GLOBAL env id and ups + downs alone: shard-invariant); else k
 *                                                         stays. In all three cases mark_x = root_x
 *   creation-time init, dtrl_reset, restart               mark_x = spawn_x, the level stays
 * spawn_x is the root x a reset leaves (the character file's default pose, or -init_pos_x=). The rule looks at nothing else: no exploration, reward, episode
 * distance or other env. With -terrain_gen= device it runs inside the boundary launch the batch already queues per env group and frame (no host round trip, no
 * launch more; dtrl_run_frames and the overlapped loops included); in host terrain mode in the host's per-frame status loop. It also runs at the boundary behind
 * dtrl_step_updates. Settings and records are batch state like the assignment: snapshots, restores, clones and blobs leave them alone -- a restored env that now
 * stands behind its mark_x therefore counts as "early" at its next fall. Timing as the terrain calls above. */
/* No counterpart in the reference, which keeps one terrain per scene object. Create or replace the batch's ladder: every env's mark_x becomes its current root x, the counters go to 0, the levels
 * stay. lo > hi removes the ladder (the levels stay where they are). DTRL_ERR_ARG: no terrain set, lo / hi out of range, an empty terrain inside [lo, hi],
 * up_dist <= 0, down_dist < 0, at_top not 0 / 1, model variants whose spawn x differ, a frame in flight. */
dtrl_status dtrl_terrain_ladder(dtrl_batch* b, int lo, int hi, double up_dist, double down_dist, int at_top);
/* No counterpart in the reference, which keeps one terrain per scene object. The ladder records of the listed envs (env_ids == NULL: the first n), as of the last completed boundary: refused between
 * dtrl_step_begin and dtrl_step_end, otherwise waits for queued work. Any output may be NULL. With a ladder present dtrl_assign_terrains keeps working: restart
 * != 0 puts the listed envs' mark_x to spawn_x, restart == 0 to the env's current root x; the counters stay. */
dtrl_status dtrl_ladder_info(dtrl_batch* b, const int32_t* env_ids, int n, double* mark_x_out, int32_t* ups_out, int32_t* downs_out);

/* Replaces: cScenarioSimChar::AddPerturb -> cWorld::AddPerturb (scenarios/ScenarioSimChar.cpp:204-207, sim/World.cpp:256-259) with a
 * tPerturb of type ePerturbForce (sim/Perturb.cpp:52-79, sim/World.cpp:445-470): a world-frame force[n][2] on body part link[n] at the
 * body-local offset local_pos[n][2] (NULL = the COM) for duration[n] seconds of simulated time, advanced and applied at the start of
 * every env-step like cPerturbManager::UpdatePerturbs. One slot per env (a new perturbation replaces the old one); reset clears it. An env listed
 * several times keeps its last row. The rows reach the slots in one launch. */
dtrl_status dtrl_add_perturb(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* link, const double* local_pos, const double* force, const double* duration);
/* Replaces: cScenarioSimChar::ApplyRandForce() (scenarios/ScenarioSimChar.cpp:209-235; ranges -min_perturb= -max_perturb=
 * -min_pertrub_duration= -max_perturb_duration= as the reference spells them): a random body part, direction, magnitude and duration per
 * env. The reference draws from its time-seeded global RNG; here the draw is a function of (seed, global env id). */
dtrl_status dtrl_apply_rand_force(dtrl_batch* b, const int32_t* env_ids, int n, uint64_t seed);

/* ---- Push schedule: random external pushes on the device at per-env random times (robustness training and evaluation) ----
 * No counterpart in the reference as a schedule: its scenarios call ApplyRandForce by hand (a key press). Replaces: cScenarioSimChar::ApplyRandForce
 * (scenarios/ScenarioSimChar.cpp:209-235) called from a host loop. A schedule is a range of waits [min_wait, max_wait] counted in the env's frame boundaries, a
 * range of force magnitudes and of durations, and a seed. Each env carries a record (wait, ctr, pushes, the last push) and a scale (1.0 unless set). The draws of
 * env e are u(i) = (bits(i) >> 11) * 2^-53 with bits(i) = mix(mix(mix(seed) ^ (C + global env id)) + i * 0xD1342543DE82EF95), i = ctr++ for every draw: mix is
 * the terrain streams' 64-bit finaliser, C a constant of the schedule's own, the global env id -env_id_base= + local id. The stream is shard-invariant and
 * independent of exploration, reward and every other env. At env e's FRAME BOUNDARY (behind every dtrl_step / dtrl_step_end / frame of dtrl_run_frames /
 * dtrl_step_updates), in this order:
 *   scale[e] == 0           nothing: the env is not in the schedule, nothing of it is read, drawn or written (evaluation envs are held out this way)
 *   an episode starts       (the env fell in this frame; dtrl_push_schedule itself; dtrl_reset naming it, once however often it is listed; dtrl_assign_terrains
 *                           with restart != 0) wait = min_wait + floor(u * (max_wait - min_wait + 1)), clamped to max_wait. No push.
 *   else                    wait -= 1; while it is still > 0 nothing more
 *   wait reached 0          a push, drawn in ApplyRandForce's order: link floor(u * L) (clamped to L - 1); three (sign, magnitude) pairs d = +-u (sign: u < 0.5 is
 *                           -1), normalised, (1, 0, 0) standing in for a zero vector, x and y kept; f = scale * (min_force + u * (max_force - min_force)) * d / |d|;
 *                           dur = min_dur + u * (max_dur - min_dur). The env's perturbation slot is written as dtrl_add_perturb writes it for a push at the
 *                           link's COM, the push is recorded, pushes += 1, and the next wait is drawn.
 * Every value is computed in double in both libraries and cast to the library's arithmetic type only where it is stored into the slot. A push never happens at an
 * episode start, so nothing depends on whether the rule runs in front of or behind the reset that clears the slot. A scheduled push and dtrl_add_perturb share
 * the env's one slot: the later writer wins, as in the reference's manager. The rule is one small launch per env group and frame on the group's stream in both
 * terrain modes (no host wait is added; dtrl_run_frames and the overlapped loops included); a batch without a schedule queues what it always queued. It combines
 * with policy slots, model variants and their redraw, terrain sets and the ladder. NOT available with -policy_mode= external: a parked env's boundaries are not
 * frames, a wait counted in ticks would depend on the caller's pace. Settings, records and scales are batch state: snapshots, restores, clones and blobs leave
 * them alone (the slot itself is part of the env's state and travels as it always has). */
/* No counterpart in the reference / Replaces: cScenarioSimChar::ApplyRandForce (scenarios/ScenarioSimChar.cpp:209-235). Turn the schedule on or replace its
 * settings (1 <= min_wait <= max_wait; every env of scale != 0 draws a first wait under them), or remove it (min_wait > max_wait). Records, counters and scales
 * are kept in all three cases. NaN for any of the four ranges means the batch's -min_perturb= -max_perturb= -min_pertrub_duration= -max_perturb_duration=.
 * DTRL_ERR_ARG, nothing changed: min_wait < 1, a negative or infinite range, min > max, -policy_mode= external, a frame in flight. */
dtrl_status dtrl_push_schedule(dtrl_batch* b, int min_wait, int max_wait, uint64_t seed, double min_force, double max_force, double min_dur, double max_dur);
/* No counterpart in the reference / Replaces: cScenarioSimChar::ApplyRandForce (scenarios/ScenarioSimChar.cpp:209-235). scales[i] -> env_ids[i] (env_ids == NULL:
 * the first n envs): finite and >= 0, all or nothing (DTRL_ERR_ARG, nothing changed). 0 takes the env out of the schedule, any other value multiplies its force
 * (one batch can hold a magnitude sweep). May be called before dtrl_push_schedule. An env that comes in from 0 while a schedule runs has not drawn a wait: it
 * is pushed at its next boundary and follows the schedule from there. Refused while a frame is in flight. */
dtrl_status dtrl_push_scale(dtrl_batch* b, const int32_t* env_ids, int n, const double* scales);
/* No counterpart in the reference / Replaces: cScenarioSimChar::ApplyRandForce (scenarios/ScenarioSimChar.cpp:209-235). Per listed env (env_ids == NULL: the
 * first n): boundaries left until its next push, pushes so far, and the last push as drawn (link, -1 = none yet; force[n][2]; duration), as of the last completed
 * boundary: refused between dtrl_step_begin and dtrl_step_end and before the first dtrl_push_schedule / dtrl_push_scale, otherwise waits for queued work. Any
 * output may be NULL. */
dtrl_status dtrl_push_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* wait, int32_t* pushes, int32_t* last_link, double* last_force, double* last_dur);
/* ---- Episode limits: end episodes by time or distance, on the device ----
 * No counterpart in the reference: its episodes end by a fall alone (`scenarios/ScenarioExp.cpp:83-98`, `scenarios/ScenarioPoliEval.cpp:110-125`). With a limit, an
 * env whose episode has lasted a per-episode drawn number of frame boundaries, or has travelled max_dist from the spawn x, ends its episode at that boundary as if
 * it had fallen -- without a DTRL_TUPLE_FAIL tuple and without the host. Each env carries a record (frames, limit, draws, the last episode, by_fall, by_limit) and a
 * flag (1 unless set; 0 holds the env out: nothing of it is read, drawn or written). The limit of an episode is limit = min_frames + floor(u * (max_frames -
 * min_frames + 1)), clamped to max_frames, with u = (bits >> 11) * 2^-53, bits = mix(mix(mix(seed) ^ (C + global env id)) + draws++ * 0xD1342543DE82EF95): mix is
 * the terrain streams' 64-bit finaliser, C a constant of the limit's own, the global env id -env_id_base= + local id. A range rather than one number, so that
 * lock-stepped envs do not all reset in the same frame. min_frames == max_frames == 0: no frame limit, nothing is drawn, limit is 0. At env e's FRAME BOUNDARY (the
 * boundaries the push schedule counts), in front of every other boundary rule:
 *   flag[e] == 0              nothing
 *   the env fell              frames += 1, by_fall += 1, the episode is recorded (last_frames, last_dist = root_x - spawn_x, last_cause 1); frames = 0, a new limit.
 *                             A fall wins over a limit reached in the same frame.
 *   else                      frames += 1; limit > 0 and frames >= limit: cause 2; else root_x - spawn_x >= max_dist: cause 3. Either: by_limit += 1, the episode is
 *                             recorded, frames = 0, a new limit, and the env's episode ENDS: need_reset is written into its status record and its state, in the
 *                             poli_eval scenario with num_cycles >= 1 together with what a fall does there (dist = q[0] - pos_start_x, the avg_dist / num_episodes
 *                             update, the distance log entry), computed in the library's arithmetic type.
 * An episode also starts, without a boundary (frames = 0, a new limit), when the limit is set, when dtrl_reset names the env (once however often it is listed), on
 * dtrl_assign_terrains with restart != 0, and when the env's flag goes from 0 to 1 while a limit runs. For every rule behind it the env is one whose episode ended:
 * the terrain ladder puts its mark back to the spawn x (and moves the env down only if it is less than down_dist past its mark), redraw and rescale draw, the push
 * schedule draws a wait, the terrain work builds a fresh window, and the reset launch resets it under the new model. The tuple in progress is dropped, as dtrl_reset
 * on a running env drops it. The rule is one small launch per env group and frame on the group's stream in both terrain modes: no host wait is added
 * (dtrl_run_frames and the overlapped loops included), and a batch without a limit queues what it always queued. dtrl_eval_stats' resets goes on counting every
 * reset; by_fall / by_limit split them by cause. Settings, records and flags are batch state: snapshots, restores, clones and blobs leave them alone. */
/* No counterpart in the reference: its episodes end by a fall alone (`scenarios/ScenarioExp.cpp:83-98`, `scenarios/ScenarioPoliEval.cpp:110-125`). Sets the limit,
 * replaces it (every env under it starts an episode: frames 0, a new limit) or removes it (min_frames == max_frames == 0 and max_dist +inf or <= 0). max_dist +inf
 * or <= 0: no distance limit. Records, counters and flags are kept in all three cases. spawn_x is the x a reset leaves in q[0]. DTRL_ERR_ARG, nothing changed:
 * min_frames < 0, min_frames > max_frames, exactly one of the two is 0, NaN, -policy_mode= external (a parked env's boundaries are ticks), a frame in flight. */
dtrl_status dtrl_episode_limit(dtrl_batch* b, int min_frames, int max_frames, double max_dist, uint64_t seed);
/* No counterpart in the reference: its episodes end by a fall alone (`scenarios/ScenarioExp.cpp:83-98`, `scenarios/ScenarioPoliEval.cpp:110-125`). on[i] -> the flag
 * of env_ids[i] (env_ids == NULL: the first n envs), all or nothing (DTRL_ERR_ARG, nothing changed); an env listed twice keeps its last flag. May be called before
 * dtrl_episode_limit. An env that comes in (0 -> 1) while a limit runs starts an episode record at this call. Refused while a frame is in flight. */
dtrl_status dtrl_episode_limit_envs(dtrl_batch* b, const int32_t* env_ids, int n, const uint8_t* on);
/* No counterpart in the reference: its episodes end by a fall alone (`scenarios/ScenarioExp.cpp:83-98`, `scenarios/ScenarioPoliEval.cpp:110-125`). Per listed env
 * (env_ids == NULL: the first n): the record as of the last completed boundary -- boundaries of the running episode, its limit (0: none), episodes ended by a fall
 * and by a limit, and the last ended episode's length, root_x - spawn_x and cause (1 fall, 2 frame limit, 3 distance; 0 none yet). Refused between dtrl_step_begin
 * and dtrl_step_end and before the first dtrl_episode_limit / dtrl_episode_limit_envs, otherwise waits for queued work. Any output may be NULL. */
dtrl_status dtrl_episode_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* frames, int32_t* limit, int64_t* by_fall, int64_t* by_limit, int32_t* last_frames, double* last_dist, int32_t* last_cause);
/* ---- frame trace: per-frame state rows of chosen envs, recorded on the device ----
 * The reference looks at a run through its GUI, or by cCharacter::WriteState once per frame (`anim/Character.cpp:217-262`); here hundreds of frames are queued
 * without the host looking at the batch (dtrl_run_frames, dtrl_step_poll, -terrain_gen= device), and every getter is a blocking copy of a whole EnvState per listed
 * env BETWEEN frames -- by which time an env that fell has been reset. The trace is a ring of `frames` compact rows per traced env in device memory. At every FRAME
 * BOUNDARY of an env group (the boundaries the episode limit counts), behind the group's frame launch and the episode limit and in front of the terrain work, the
 * ladder, redraw, rescale, push and the reset launch, each traced env of the group that completed a frame in that launch writes one row into slot rows_written %
 * frames of its own ring, then rows_written += 1 (a counter per env: the groups' streams need no common frame number). In -policy_mode= external "completed a
 * frame" is ext_steps_left == 0 behind the tick: a parked env writes nothing. So a row shows the state the frame ended in -- a fallen pose included --, its
 * need_reset is what everything queued behind it sees (a limit's truncation included), and its keys are the ones the frame ran under. The listed episode starts
 * (dtrl_reset, a terrain restart, the creation of a rule) write no row. A row is W = 3 D + 2 doubles -- time, phase, q[D], qd[D], tau[D] (the clamped torques held
 * for the next world update); the fp32 library converts each value exactly, as its getters do -- and 12 int32: row (the env's rows_written before the write),
 * need_reset (the status record's), action_id, state, stance, contact_bits, the low words of num_cycles and num_resets, slot, variant, terrain (the env's key in
 * each family as the device holds it at that moment, 0 without a table; a private rescale key reads V + e, as in dtrl_get_variants), 0 (reserved). One small launch
 * per env group and frame over the group's own list of traced envs, on the group's stream in both terrain modes; a group without a traced env, and a batch without
 * a trace, queue what they always queued. Ring, counters and lists are batch state: snapshots, restores, clones, blobs and resets leave them alone. */
/* Replaces: cCharacter::WriteState called once per frame (`anim/Character.cpp:217-262`), and the GUI as the only way to look at a run. Starts a trace of the n
 * listed local envs (distinct, in any order; env_ids == NULL: every env) with `frames` >= 1 rows per env. A second call replaces the trace: the old ring is freed
 * and every counter starts from 0. n == 0 removes it. Refused between dtrl_step_begin and dtrl_step_end (it never waits for a frame), then waits for every stream.
 * DTRL_ERR_ARG, nothing changed: an id out of range or listed twice, frames < 1. DTRL_ERR_CAPACITY: the ring does not fit; the batch is left without a trace. */
dtrl_status dtrl_trace(dtrl_batch* b, const int32_t* env_ids, int n, int frames);
/* Replaces: nothing the reference has (see dtrl_trace; `anim/Character.cpp:217-262`). The trace in force: traced envs (0: none), rows per ring, W (3 D + 2, also
 * without a trace), the traced env ids in dtrl_trace's order and each one's rows_written (int64 per traced env). Any output may be NULL. Refused while a frame is
 * in flight, otherwise waits for queued work. */
dtrl_status dtrl_trace_info(dtrl_batch* b, int32_t* n_traced, int32_t* frames, int32_t* width, int32_t* env_ids_out, int64_t* rows_written_out);
/* Replaces: reading back what cCharacter::WriteState wrote frame by frame (`anim/Character.cpp:217-262`; cMotion reads such frames, `anim/Motion.cpp:109-171`). For
 * each listed traced env (env_ids == NULL: all of them, in dtrl_trace's order) the last counts[i] = min(rows_written, frames, max_rows) rows, OLDEST FIRST, into
 * vals [n][max_rows][W] (double) and ints [n][max_rows][12] (int32); rows beyond counts[i] are left untouched. Refused while a frame is in flight, waits for queued
 * work and returns synchronised. DTRL_ERR_ARG: no trace, an env that is not traced. */
dtrl_status dtrl_trace_read(dtrl_batch* b, const int32_t* env_ids, int n, int max_rows, double* vals, int32_t* ints, int32_t* counts);
/* Replaces: the same read (`anim/Character.cpp:217-262`) for a consumer on the device -- an external policy's extra inputs, an asymmetric critic, a learned
 * discriminator: vals_dev / ints_dev are DEVICE pointers of the same shapes, counts is host memory. One launch unrolls the rings; nothing crosses to the host but
 * the counts. */
dtrl_status dtrl_trace_read_device(dtrl_batch* b, const int32_t* env_ids, int n, int max_rows, double* vals_dev, int32_t* ints_dev, int32_t* counts);
/* ---- episode log: one row per ended episode, recorded on the device ----
 * The nearest thing the reference has is cScenarioPoliEval's distance log (`scenarios/ScenarioPoliEval.cpp:202-217` RecordDistTraveled into mDistLog, read by
 * GetDistLog `:147-150`): one distance per episode and nothing else. Here every per-episode rule of the frame boundary (variant redraw, rescale, push schedule,
 * terrain ladder, episode limit) acts on the device with no host wait, and dtrl_episode_info / dtrl_get_variants / dtrl_variant_rescale_info refuse a frame in
 * flight, wait for every stream, hold the last episode alone and are read after the boundary has redrawn keys and scales. The episode log is a ring of 64-byte rows
 * per ENV GROUP (one stream each: no atomics, no order between streams) in page-locked host memory the device writes. At every FRAME BOUNDARY of a group (the
 * boundaries the episode limit and the trace count; dtrl_step_updates counts), behind the group's frame launch, the episode limit and the trace and in front of
 * the terrain work, the ladder, redraw, rescale, push and the reset launch, every env of the group that completed a frame (-policy_mode= external: ext_steps_left
 * == 0 behind the tick; a parked env counts nothing) counts the boundary, and one whose status record has need_reset != 0 appends a row, in ascending env id, at
 * slot (written + k) % capacity; then its ordinal rises and its frame and cycle counts start over. Of more than `capacity` rows in one boundary the last
 * `capacity` are stored; the group's cursor counts every row. The listed episode starts (dtrl_reset, a terrain restart) abandon the running episode without a row.
 * One launch of one workgroup per env group and frame; a batch without a log queues what it always queued. Rings, cursors and the per-env records are batch
 * state: snapshots, restores, clones, blobs and resets leave them alone. Also available with -policy_mode= external, where no episode limit exists. */
typedef struct dtrl_episode_row {
	int32_t env, cause, frames, cycles;       /* local env id; 1 fall, 2 frame limit, 3 distance; frame boundaries the episode saw; num_cycles at its end minus at its start */
	int64_t boundary, episode;                /* the group's boundary counter at which the episode ended (0-based since the log was set); the env's ordinal 0, 1, 2 ... */
	double dist; int32_t need_reset, zero;    /* root_x - spawn_x at the end (dtrl_episode_info's last_dist); the status record's need_reset as every later rule sees it; 0 */
	int32_t slot, variant, terrain, rescale_draw;   /* the env's keys as the device holds them while the episode ran (0 without a table; a private rescale key reads V + e); the
	                                                   draw number n of the episode's rescale factors (dtrl_variant_rescale_factors), -1 for an env not under its private key */
} dtrl_episode_row;
/* Replaces: cScenarioPoliEval::RecordDistTraveled's mDistLog (`scenarios/ScenarioPoliEval.cpp:202-217`) as the only per-episode record. Sets or replaces the log:
 * `capacity` >= 1 rows per env group; cursors, boundary counters and per-env records start from 0, and every env's first logged episode starts at this call (its
 * cycles count from the env's cycle counter as it stands). capacity == 0 removes the log. Refused between dtrl_step_begin and dtrl_step_end (it never waits for a
 * frame), then waits for every stream. DTRL_ERR_ARG, nothing changed: capacity < 0. DTRL_ERR_CAPACITY: a ring cannot be allocated; the batch is left without a log. */
dtrl_status dtrl_episode_log(dtrl_batch* b, int32_t capacity);
/* Replaces: nothing the reference has (see dtrl_episode_log; `scenarios/ScenarioPoliEval.cpp:147-150`). Totals over the env groups: rows per ring (0: no log), the
 * number of rings, rows ever appended, and rows overwritten before a drain took them. Any output may be NULL. Refused while a frame is in flight, otherwise
 * waits for queued work. */
dtrl_status dtrl_episode_log_info(dtrl_batch* b, int32_t* capacity, int32_t* n_groups, int64_t* written, int64_t* lost);
/* Replaces: cScenarioPoliEval::GetDistLog (`scenarios/ScenarioPoliEval.cpp:147-150`). The rows not drained yet, merged over the groups in (boundary, env) order,
 * at most max_rows of them into out; the rest stay for the next call. *n: rows returned; *lost (may be NULL): rows this call found overwritten before it could
 * take them. NEVER queues GPU work. With no frame in flight it first waits for queued work, as the info calls do (with -terrain_gen= device dtrl_step returns with
 * the boundary still queued); between dtrl_step_begin and dtrl_step_end it does not wait and returns what has been published so far. Per group the host reads
 * the cursor, copies the rows behind its own mark, then reads the cursor and the writer's reservation again and drops every copied row whose slot a later boundary
 * has taken or is taking. DTRL_ERR_ARG: no log, max_rows < 0. */
dtrl_status dtrl_episode_log_drain(dtrl_batch* b, dtrl_episode_row* out, int32_t max_rows, int32_t* n, int64_t* lost);
/* Replaces: nothing the reference has (`scenarios/ScenarioPoliEval.cpp:202-217` logs a distance, no model). The rescale's rule on the host for arbitrary (env,
 * draw) pairs: factors [n][4][L] in dtrl_variant_rescale_info's layout, the factors env env_ids[i] drew for its draw number draws[i] (a row's rescale_draw); draw
 * -1 gives all 1. What dtrl_variant_rescale_info does for the current episode alone. Needs no wait. DTRL_ERR_ARG: no rescale, an id out of range, a draw < -1. */
dtrl_status dtrl_variant_rescale_factors(dtrl_batch* b, const int32_t* env_ids, const int32_t* draws, int32_t n, double* factors);
/* Replaces: cNNController::RecordPoliState (sim/TerrainRLCharController.cpp:120-123). */
dtrl_status dtrl_get_poli_state(dtrl_batch* b, const int32_t* env_ids, int n, double* s);
/* Replaces: cNeuralNet::GetLayerState("output", y) (learning/NeuralNet.cpp:814-834) after the controller's last cNeuralNet::Eval
 * (learning/NeuralNet.cpp:352-375; what -record_nn_activation= true -nn_activation_layer= output writes, scenarios/ScenarioPoliEval.cpp:271-286)
 * with the output un-normalisation of Eval applied: y[n][nn_out of dtrl_dims] = the net's outputs of each env's most recent action decision
 * that evaluated the net (zeros before the first one). */
dtrl_status dtrl_get_policy_output(dtrl_batch* b, const int32_t* env_ids, int n, double* y);
/* fallen | stumbled<<1 | new_cycle<<2 | fsm_state<<8: cSimCharacter::HasFallen/HasStumbled, cCharController::IsNewCycle/GetState. */
dtrl_status dtrl_get_flags(dtrl_batch* b, const int32_t* env_ids, int n, uint32_t* bits);
/* Replaces: cSimCharacter::GetBodyPart(i)->GetPos() / GetLinearVelocity() / GetRotation() (sim/SimCharacter.cpp:317-352, sim/SimObj.cpp:
 * 60-130), what the reference's features, recorders and draw code read per link: world position and velocity of every link's body
 * COM ([n][L][2] each) and the body's world angle ([n][L]); derived from (q, qd) with the same planar kinematics the kernel uses.
 * Any output may be NULL. */
dtrl_status dtrl_get_link_states(dtrl_batch* b, const int32_t* env_ids, int n, double* com_xy, double* com_vel_xy, double* angle);

/* observability for parity tests: controller torque before / after the cJoint clamp (sim/Joint.cpp:171-201), per-link contact flags */
dtrl_status dtrl_get_torques(dtrl_batch* b, const int32_t* env_ids, int n, double* tau_ctrl, double* tau_applied);
dtrl_status dtrl_get_contacts(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* flags);
/* current action: cTerrainRLCharController::GetCurrActionID + mCurrAction.mParams, PD targets */
dtrl_status dtrl_get_ctrl(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* state, double* phase, int32_t* action_id, double* params, double* pd_targets);
/* What cScenarioPoliEval's per-cycle recorders read (scenarios/ScenarioPoliEval.cpp:234-404: RecordAction, RecordVel, RecordActionIDState): the
 * env's cycle counter (mCycleCount; like the reference's it survives resets) and reset counter, the COM and simulated time at the start of the current cycle (what mChar->CalcCOM() / mTime returned when
 * the cycle began), and the optimisable parameters of the current action (cTerrainRLCharController::BuildOptParams, [n][frag_size] as dtrl_dims reports it). The action id is in
 * dtrl_get_ctrl, the policy state of the current action in dtrl_get_poli_state. deepterrainrl_amd.recorders.PoliEvalRecorder writes the
 * reference's files from these at frame boundaries (all of them are constant over a cycle, so nothing is lost). Any output may be NULL. */
dtrl_status dtrl_get_cycle_info(dtrl_batch* b, const int32_t* env_ids, int n, int64_t* num_cycles, int64_t* num_resets, double* cycle_start_com, double* cycle_start_time, double* opt_params);
/* Replaces: cTerrainRLCharController::BuildActionOptParams(a) for every action a (what cScenarioPoliEval::InitActionRecord writes): table[n_actions][frag_size];
 * returns the number of actions through n_actions (table may be NULL to query it). */
dtrl_status dtrl_get_action_table(dtrl_batch* b, int* n_actions, double* table);
/* ground observability: cGround::SampleHeight (sim/GroundVar2D.cpp:98-114) with the grid cell it used (terrain-index parity) */
dtrl_status dtrl_sample_ground(dtrl_batch* b, int env, int n, const double* x, double* h, int32_t* seg, int32_t* i, int32_t* j);
/* Replaces: cGroundVar2D::GetSegment(s) / tSegment::mData, GetMinX / GetMaxX (sim/GroundVar2D.cpp:279-290, 392-455, 504-520) of one env's two-segment
 * window in logical order (slot 0 = min segment): vertex counts, x ranges, and the heights (metres, float) of each slot, heights0 / heights1 holding
 * up to cap values each (may be NULL). num_builds = segments built for this env so far (-terrain_gen= device; -1 in host mode) */
dtrl_status dtrl_get_ground_window(dtrl_batch* b, int env, int32_t* w2, double* min_x2, double* max_x2, float* heights0, float* heights1, int cap, int64_t* num_builds);

/* Replaces: cScenarioPoliEval::GetAvgDist / GetNumEpisodes / GetNumCycles (scenarios/ScenarioPoliEval.h:20-26), batch aggregate. */
dtrl_status dtrl_eval_stats(dtrl_batch* b, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);

/* Replaces: cScenarioPoliEval::GetDistLog (scenarios/ScenarioPoliEval.cpp:147-150, filled by RecordDistTraveled :202-217) for the batch: the distance of
 * every recorded episode since creation, grouped by env id (= pool member, the order cOptScenarioPoliEval::OutputResults walks,
 * optimizer/scenarios/OptScenarioPoliEval.cpp:213-239), each env's episodes in time order. *out_n = number of entries (call with cap 0 and
 * NULL buffers to size them). */
dtrl_status dtrl_get_dist_log(dtrl_batch* b, double* dist, int32_t* env_ids, int cap, int* out_n);
/* Replaces: cScenarioPoliEval::ResetAvgDist (scenarios/ScenarioPoliEval.cpp:132-136) on every env: average distance and episode count restart,
 * cycle counters and the dist log stay (cOptScenarioPoliEval::EvalHelper calls it after folding a batch of episodes into its record, :184-196). */
dtrl_status dtrl_reset_avg_dist(dtrl_batch* b);
/* Replaces: cOptScenarioPoliEval::OutputResults (optimizer/scenarios/OptScenarioPoliEval.cpp:213-239): appends ONE line to `path`, every logged
 * distance in dtrl_get_dist_log order, printed with std::to_string and separated by ", ". */
dtrl_status dtrl_write_dist_log(dtrl_batch* b, const char* path);

/* sizes: L links, D dofs, S policy-state, A policy-action (1 + frag), P controller params, nn_out, num_frags, frag_size */
dtrl_status dtrl_dims(const dtrl_batch* b, int* L, int* D, int* S, int* A, int* P, int* nn_out, int* num_frags, int* frag_size);

/* HIP stream the batch launches on (so callers can bracket it with their own events), and the last kernel timing:
 * average duration in ms of the frame kernel over the launches since the previous call, measured with hipEvents on that stream. */
dtrl_status dtrl_kernel_time_ms(dtrl_batch* b, double* avg_ms, int64_t* launches);

/* ---- host-side pieces of the path that need no batch and no device (the reference's static / utility entry points) ---- */

/* Replaces: cTerrainGen2D::ParseType + GetTerrainFunc(type) (sim/TerrainGen2D.cpp:90-181) called as func(width, params, rand, data) on a
 * cRand seeded with `seed` (util/Rand.cpp:89-92), i.e. what cGroundVar2D::BuildSegment runs per segment (sim/GroundVar2D.cpp:312-342).
 * params40 in cTerrainGen2D::eParams order (sim/TerrainGen2D.h:31-81). The strip (float heights, 0.1 m vertex spacing) is written to
 * out[0..min(n, cap)); *out_n = vertex count, *out_width = the function's return value (metres added). Bit-identical to the reference
 * on the same libstdc++. */
dtrl_status dtrl_terrain_build(const char* type_name, const double* params40, uint64_t seed, double width, float* out, int cap, int* out_n, double* out_width);
/* Replaces: the terrain-file reader of cScenarioSimChar::ParseTerrainParams (scenarios/ScenarioSimChar.cpp:670-706) + cTerrainGen2D::LoadParams
 * (sim/TerrainGen2D.cpp:69-81): "Type" string and every 40-vector of the "Params" array (defaults sim/TerrainGen2D.cpp:8-56). */
dtrl_status dtrl_terrain_load_file(const char* path, char* type_out, int type_cap, double* params_out, int max_sets, int* out_sets);
/* Replaces: cArgParser(argv, argc) + AppendArgs(-arg_file) + ParseString(key) (optimizer/Main.cpp:19-32, util/ArgParser.cpp:42-108, 131-150) exactly as
 * dtrl_create resolves its arguments (-data_root= prefixes a relative -arg_file=). *found = 0 when the key is absent or followed by another key.
 * Returns the number of tokens through n_tokens (may be NULL). */
dtrl_status dtrl_args_parse_string(const char* const* argv, int argc, const char* key, char* out, int cap, int* found, int* n_tokens);

const char* dtrl_last_error(const dtrl_batch* b);
const char* dtrl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DTRL_H_ */
