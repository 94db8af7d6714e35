/*
 * libtoricenv -- C-ABI of the MI355X-native batched toric-code environment.
 *
 * This is the drop-in boundary for the reference's env hot path.  The reference has no
 * FFI of its own (pure Python duck typing); each entry point below names the Python
 * interface it replaces (paths relative to the upstream tree).  A reference-side ctypes
 * binding is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (TQ_E_*); tq_last_error() gives
 *    the message of the calling thread's last failure.  Nothing aborts.
 *  - all array arguments are DEVICE pointers owned by the caller (e.g. a PyTorch-ROCm
 *    tensor's data_ptr()) unless the name says "host".  The library owns only the
 *    per-handle lattice state.  No allocation and no synchronisation happens on the hot
 *    path: kernels are enqueued on `stream` (a hipStream_t, NULL = default stream) and
 *    the call returns.
 *  - lattices are (2,d,d): [0] = vertex matrix, [1] = plaquette matrix (src/util.py:63-64);
 *    qubit codes I=0 X=1 Y=2 Z=3 (docs/toric_model.md:11); action = [layer,row,col,op],
 *    op in 1..3 (src/util.py:10, src/numba/util_actor.py:100-104).
 *  - a handle is not thread-safe; use one handle per process / GPU
 *    (one actor process per device: Distributed_mp.py:201-211).  Entry points make the handle's
 *    device current while they run and restore the caller's device before returning.
 *  - set-up calls (tq_create, tq_destroy, tq_set_perror_schedule, tq_states_reserve, the first use of a
 *    lattice size on a device) allocate and synchronise; everything else only enqueues kernels.
 *    tq_create, tq_destroy and tq_states_reserve leave the caller's current device unchanged.
 *  - tq_states_persp_count / tq_states_persp_write use one per-device scratch area sized by
 *    tq_states_reserve (they return TQ_E_CAPACITY when it is too small, they never allocate); calls
 *    that use it must be issued on one stream or be separated by a synchronisation.
 *  - alignment: `actions`, `actions_out`, `offsets`, `counts`, `positions` and the stack `out` are
 *    accessed with 16-byte vector loads/stores and must be 16-byte aligned (TQ_E_INVALID otherwise;
 *    any hipMalloc / PyTorch allocation is).  For full store bandwidth `out` and `positions` should
 *    be 128-byte aligned (tq_persp_write writes whole 128-byte lines).  A row of a 2-D int64 offsets
 *    array needs an even row length.
 *  - RNG: counter-based Philox4x32-10 keyed (seed, global env id, episode, round/step);
 *    contract in DESIGN.md.  Results are identical for any partition of env ids over GPUs.
 */
#ifndef TORICENV_H
#define TORICENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TQ_VERSION 200      /* 200: packed block carries f32 priority; every slot written (op 0 = no transition) */

#define TQ_OK 0
#define TQ_E_INVALID (-1)   /* bad argument (NULL handle, even d, unsupported d, n <= 0 ...) */
#define TQ_E_HIP (-2)       /* a HIP runtime call failed; message in tq_last_error() */
#define TQ_E_CAPACITY (-3)  /* output capacity too small */
#define TQ_E_ACTION (-4)    /* an action outside the lattice / op not in 1..3 was seen on the device */
#define TQ_E_INDEX (-5)     /* tq_reset_idx saw an index out of range or listed twice (latched, tq_check) */
#define TQ_E_RESET (-6)     /* a reset hit the round limit without producing a defect (latched, tq_check) */

/* element type of the perspective stack written by tq_persp_write */
#define TQ_F32 0            /* float32 -- what the reference feeds the NN (numba/util_actor.py:39) */
#define TQ_F16 1
#define TQ_BF16 2
#define TQ_U8 3

/* p_error strategy of the fused auto-reset (Actor_mp.py:176-180) */
#define TQ_PERR_FIXED 0     /* every reset uses p_error_default */
#define TQ_PERR_LINEAR 1    /* roof = min(final, roof + delta); p = roof */
#define TQ_PERR_RANDOM 2    /* roof as above; p ~ U(start, roof) */

typedef struct tq_env tq_env;

int tq_version(void);
const char* tq_last_error(void);

/* gym.make('toric-code-v0', config={"size","min_qubit_errors":0,"p_error"}) + EnvSet(env, no_envs)
 * (Distributed_mp.py:72-76, src/EnvSet.py:5-16).  d odd in {3,5,...,21}.  Lattice e of this
 * handle has global env id first_env_id + e (shard offset for multi-GPU). */
int tq_create(tq_env** out, int n_envs, int d, int device, uint64_t seed, int64_t first_env_id);
int tq_destroy(tq_env* h);

/* env config: default p_error in (0,1] (gym config "p_error"), terminal reward (default 100,
 * evaluation.py:175), max_actions_per_episode (default 75, Distributed_mp.py:44; used only by
 * tq_actor_step's auto-reset).  p_error = 0 is rejected (a reset could never produce a defect) unless the
 * fixed-n sampler was selected first with tq_set_min_qubit_errors(n > 0), which does not use p_error. */
int tq_set_params(tq_env* h, double p_error_default, double terminal_reward, int max_steps_per_episode);
/* gym config "min_qubit_errors": 0 (default, every config of the reference tree) = depolarizing
 * sampler at p_error; n > 0 = every reset places exactly n errors on uniformly chosen distinct
 * qubits with uniform Paulis (the fixed-n sampler, results/small_p_error_test.py:34-40; p_error
 * is then unused), still redrawn until the syndrome is non-empty. */
int tq_set_min_qubit_errors(tq_env* h, int n_errors);
/* p_error schedule of the actor's reset policy (Actor_mp.py:41-46,176-180) for tq_actor_step. */
int tq_set_perror_schedule(tq_env* h, int strategy, double p_start, double p_final, double p_delta);

/* Set-up helper for the caller-owned stack buffer (np.concatenate's result, numba/util_actor.py:37-39, written every
 * step).  On MI355X a buffer has a write rate of its own for every write stream into it -- the stack write, a plain
 * fill, hipMemset -- between 5.2 and 6.9 TB/s, different from allocation to allocation and from box to box; plain
 * hipMalloc / torch.empty buffers were the slow kind in every PyTorch process of round 3 (5.1-5.5 TB/s), buffers made
 * of 2 MiB physical chunks (HIP virtual memory API) the fast kind in most (profiles/r03_stack_write_ab.txt).
 * tq_stack_alloc returns device memory of at least `bytes` bytes made of such chunks, each mapped once behind one
 * virtual range, zero-filled, and CHECKED: every 2 MiB page is verified to be reached through its own address (this
 * API leaves stale address translations behind when addresses are re-used; the library never re-uses one, never gives
 * an address range back, and does not hand out a buffer that fails the check).  Allocates, maps and synchronises; any
 * other device allocation works as `out` of tq_persp_write just as well. */
int tq_stack_alloc(int device, uint64_t bytes, void** out);
/* Gives the physical chunks back (synchronises the device first).  The VIRTUAL ADDRESS RANGE IS NEVER RETURNED: by
 * design every tq_stack_alloc leaks its 2 MiB-rounded address range for the life of the process (a re-used range
 * reaches the previous tenant's pages through stale translations on ROCm 7.2), out of a 128 TiB address space --
 * a set-up call, not something to call per step. */
int tq_stack_free(void* ptr);

/* The stack write runs one persistent workgroup per CU, each with a fixed contiguous share of the stack, dealt to the
 * XCDs round-robin.  On MI355X the CUs of the odd XCDs store this stream ~20 % slower than those of the even ones (every
 * box and buffer measured: profiles/r04_workgroup_end_times.txt), so of every pair of neighbouring workgroups the one on
 * an even XCD takes 32 + bias and the other one 32 - bias of the pair's 64 fine parts -- for d >= 7, f32 / f16 / bf16 stacks of 64 MB and more
 * (smaller lattices and the u8 stack are bound by the producers, not by the stores: there unequal shares only cost).  Default 5 (or the
 * environment variable TORICENV_XCD_BIAS, read once); 0 = equal shares; changes the speed of tq_persp_write*, never
 * its result.  tq_set_xcd_bias is the process-wide setting, tq_env_set_xcd_bias one handle's own (-1 = follow the
 * process-wide one, the default).  EnvSet.pickStackBuffer times the caller's own write both ways and sets the HANDLE
 * to the faster. */
int tq_set_xcd_bias(int bias);   /* 0..16, else TQ_E_INVALID */
int tq_get_xcd_bias(void);
int tq_env_set_xcd_bias(tq_env* h, int bias);   /* -1..16 */
int tq_env_get_xcd_bias(const tq_env* h);       /* the setting in force for this handle */
/* Test hooks of the unequal shares.  A pair's two workgroups settle who takes the larger share over one word of device
 * memory, by the parity of the XCD each runs on; on a round-robin dispatcher the two always differ.
 * tq_debug_force_xcc_parity (process-wide): -1 = the hardware's answer (the default), 0 / 1 = every workgroup claims that
 * parity (so both of a pair prefer the same share), 2 = the parity read, inverted.  Never changes what is written.
 * tq_debug_slot_words_nonzero: waits for the device, then counts the words of the handle's eight sets that are not zero --
 * every write leaves them zero (< 0: an error code). */
int tq_debug_force_xcc_parity(int parity);      /* -1..2, else TQ_E_INVALID */
int tq_debug_slot_words_nonzero(tq_env* h);

int tq_num_envs(const tq_env* h);
int tq_size(const tq_env* h);

/* EnvSet.resetAll(p_errors) (EnvSet.py:29-36): p_err = device f64[N] or NULL (default p). */
int tq_reset_all(tq_env* h, const double* p_err, void* stream);
/* EnvSet.resetTerminalEnvs(idx, p_errors) (EnvSet.py:19-27): idx = device i32[n_idx] (distinct,
 * in range), p_err = device f64[n_idx] or NULL.  Checked on the device: an index out of range is
 * skipped, of an index listed twice only one copy resets the lattice, and TQ_E_INDEX is latched. */
int tq_reset_idx(tq_env* h, const int32_t* idx, int n_idx, const double* p_err, void* stream);

/* EnvSet.step(actions) (EnvSet.py:38-47): actions = device i32[N,4]; rewards f32[N];
 * terminals u8[N].  No auto-reset (the caller resets, Actor_mp.py:171-183).  The pre-step
 * syndrome is kept inside the handle for tq_transition_write. */
int tq_step(tq_env* h, const int32_t* actions, float* rewards, uint8_t* terminals, void* stream);

/* env.state / EnvSet.states: syndrome as u8[N,2,d,d] (0/1). */
int tq_get_state(tq_env* h, uint8_t* out, void* stream);
/* rows idx[0..n_idx) only -> u8[n_idx,2,d,d] (return value of resetTerminalEnvs). */
int tq_get_state_idx(tq_env* h, const int32_t* idx, int n_idx, uint8_t* out, void* stream);
/* env.qubit_matrix as u8[N,2,d,d] Pauli codes. */
int tq_get_qubits(tq_env* h, uint8_t* out, void* stream);
/* overwrite env.qubit_matrix and recompute env.state = createSyndromOpt(qubit_matrix)
 * (results/small_p_error_test.py:112-120, results/start_from_state.py:34-38). */
int tq_set_qubits(tq_env* h, const uint8_t* qubits, void* stream);
/* per-lattice counters: episodes started, steps taken in the current episode (u32[N] each). */
int tq_get_counters(tq_env* h, uint32_t* episodes, uint32_t* steps, void* stream);
/* env.evalGroundState() per lattice -> u8[N] (1 = no non-trivial loop). */
int tq_eval_ground_state(tq_env* h, uint8_t* out, void* stream);
/* env.isTerminalState(state) per lattice -> u8[N]. */
int tq_is_terminal(tq_env* h, uint8_t* out, void* stream);

/* generatePerspectiveBatch, step 1 (numba/util_actor.py:56-67 + cumsum :35): counts i32[N]
 * (may be NULL) and offsets i64[N+1] (exclusive scan, offsets[N] = P).  A by-product are the cut points of the batch
 * into 8192 fine parts of equal perspective count from which tq_persp_write(the same `offsets` pointer) makes its 256
 * workgroups' shares; the handle keeps the tables of the last TWO calls (a write that is still running on another stream
 * reads the older one). */
int tq_persp_count(tq_env* h, int32_t* counts, int64_t* offsets, void* stream);
/* generatePerspectiveBatch + np.concatenate, step 2 (numba/util_actor.py:33-39): writes the
 * env-major stack out[P,2,d,d] of element type `dtype` and positions i32[P,3] (may be NULL)
 * for the offsets from tq_persp_count.  capacity = number of perspectives `out` can hold;
 * lattices that would overflow it are skipped and TQ_E_CAPACITY is latched (tq_check).
 * `offsets` must be the scan of the lattices' CURRENT perspective counts (tq_persp_count after the last call that
 * changed a syndrome).  The device checks it: offsets that are not (stale, shifted, all zero, decreasing, from another
 * batch) are refused -- the kernel stores nothing outside [0, min(offsets[N], capacity)) perspectives, every wait in
 * it is bounded, the grid drains, and TQ_E_INVALID is latched for tq_check; the handle stays usable.
 * At most EIGHT stack writes of one handle may be in flight at a time (on whatever streams): their workgroups take their
 * shares through a ring of eight sets of words (tq_set_xcd_bias); a write captured into a HIP graph may be replayed. */
int tq_persp_write(tq_env* h, const int64_t* offsets, void* out, int32_t* positions,
                   int64_t capacity, int dtype, void* stream);
/* The same for the lattices [first, first + count) only: `out` / `positions` receive the perspectives
 * of those lattices, the first one at index 0 (`offsets` is still the whole batch's scan), so a
 * consumer with a small buffer -- the NN forward of numba/util_actor.py:39-46 works in chunks anyway --
 * can walk a batch whose whole stack it does not want to hold (d=9: 5.3 GB per 65 536 lattices). */
int tq_persp_write_range(tq_env* h, const int64_t* offsets, int first, int count, void* out,
                         int32_t* positions, int64_t capacity, int dtype, void* stream);

/* "That stack write is done", for a second stream, without a packet of its own.  An event recorded behind a kernel
 * (hipEventRecord) is a barrier packet with a signal: ~3 us of stream time, and the next kernel of the stream starts
 * 5-7 us later than it does behind a kernel (profiles/step_fixed_cost.txt).  The _signal variants bind a library-owned
 * event to the write's own dispatch packet instead (the extended launch form of the HIP runtime with a stop event): the
 * stream carries kernel after kernel, and tq_stream_wait_event(done, other_stream) orders another stream behind the
 * write.  done == NULL: exactly tq_persp_write / tq_persp_write_range.  A stack written in several ranges passes the
 * event with the LAST range (a stream runs its kernels in order).  Not for a stream that is being captured into a HIP
 * graph (TQ_E_INVALID): a captured write is the plain tq_persp_write.  An event belongs to the device it was created
 * on; it is signalled anew by every write it is passed to, and a wait sees the latest write enqueued before it (a wait
 * for an event no write has taken yet returns at once).  create / destroy are set-up calls. */
typedef struct tq_event tq_event;
int tq_event_create(tq_event** out, int device);
int tq_event_destroy(tq_event* ev);
int tq_persp_write_signal(tq_env* h, const int64_t* offsets, void* out, int32_t* positions,
                          int64_t capacity, int dtype, tq_event* done, void* stream);
int tq_persp_write_range_signal(tq_env* h, const int64_t* offsets, int first, int count, void* out,
                                int32_t* positions, int64_t capacity, int dtype, tq_event* done, void* stream);
int tq_stream_wait_event(tq_event* ev, void* stream);

/* Same two steps for a batch of syndromes that does not live in a handle (the learner's
 * predictMaxOptimized, util_learner.py:48-111): states = device u8[n,2,d,d]. */
/* set-up: size the calling device's scratch for up to n_max states of size d (allocates, synchronises).  The
 * tq_states_persp_* calls share that ONE scratch per device: use them from one stream per device at a time. */
int tq_states_reserve(int d, int n_max);
int tq_states_persp_count(int d, int n, const uint8_t* states, int32_t* counts, int64_t* offsets,
                          void* stream);
int tq_states_persp_write(int d, int n, const uint8_t* states, const int64_t* offsets, void* out,
                          int32_t* positions, int64_t capacity, int dtype, void* stream);

/* _selectActionBatch_prime (numba/util_actor.py:69-107) on the device: q_table f32[P,3],
 * offsets i64[N+1], positions i32[P,3], eps f64[N] -> actions i32[N,4], q_values f32[N,3].
 * greedy iff (1-eps) > U; greedy = first maximum in row-major order; otherwise a uniform
 * perspective and op (Philox, keyed by the lattice's episode and step counters).
 * q_table may be NULL when every eps is 1 (pure exploration: the Q-values are never read).
 * Non-finite values -- selection (tq_select_action, tq_select_action_planned, tq_states_select_action alike).  The greedy
 * choice is np.argmax of the slice in row-major order: the first NaN if the slice holds one, else the first maximum (+inf
 * included; the first element of a slice of -inf).  q_values is the chosen row as it stands, NaN and inf included.  The
 * planned selection stays bit-identical to the dense one.  The index always lies inside the slice. */
int tq_select_action(tq_env* h, const float* q_table, const int64_t* offsets,
                     const int32_t* positions, const double* eps, int32_t* actions,
                     float* q_values, void* stream);

/* ---- The planned selection: the forward pass on the perspectives the selection reads only.  Design: DESIGN.md 3.9.
 * tq_select_action decides before it looks at a Q-value whether lattice e acts greedily -- (1-eps[e]) > U, one Philox
 * draw keyed by the lattice's (episode, step) -- and a lattice that does not reads ONE row of the Q-table (the row of the
 * perspective it drew, for q_values), a greedy lattice all n_e of its rows, a lattice without perspectives none.  Three
 * calls on one stream, with no tq_step / tq_actor_step / tq_reset_* of the handle between the first and the last:
 *   tq_select_plan            -> the list of those rows
 *   tq_nn11_forward_rows      -> q_rows f32[R][3], the Q-values of the listed rows of the stack
 *   tq_select_action_planned  -> the actions and q_values tq_select_action gives on the full table, bit for bit
 *
 * tq_select_plan: offsets i64[N+1] (tq_persp_count), eps f64[N] -> plan_offsets i64[N+1] (16-byte aligned; the exclusive
 * scan of need[e] = 0 | n_e | 1; R = plan_offsets[N], which the caller reads back to size the forward) and rows
 * i32[min(R, rows_cap)]: lattice by lattice, offsets[e] .. offsets[e+1]-1 of a greedy lattice, offsets[e] + the drawn
 * perspective of another -- strictly increasing.  rows_cap >= P always suffices.  When R > rows_cap nothing is written at
 * or past rows_cap and TQ_E_CAPACITY is latched; offsets whose differences lie outside [0, 2*d*d] latch TQ_E_INVALID
 * (tq_check reports both).  The scratch is the handle's: the call never allocates; one such call per handle at a time. */
int tq_select_plan(tq_env* h, const int64_t* offsets, const double* eps, int64_t* plan_offsets,
                   int32_t* rows, int64_t rows_cap, void* stream);
/* tq_select_action over the compact table: q_rows f32[R,3] (row i = the Q-values of perspective rows[i]), offsets and
 * positions i32[P,3] of the FULL stack, plan_offsets from tq_select_plan, the same eps -> actions i32[N,4], q_values
 * f32[N,3] (may be NULL).  It draws again with the same counters.  A lattice whose slice of the plan is not as long as this
 * eps and the handle's current counters need -- another eps, or a step between plan and selection -- gets action 0 and
 * zero q_values, reads nothing of q_rows, and TQ_E_INVALID is latched (tq_check). */
int tq_select_action_planned(tq_env* h, const float* q_rows, const int64_t* offsets,
                             const int64_t* plan_offsets, const int32_t* positions, const double* eps,
                             int32_t* actions, float* q_values, void* stream);

/* The same selection for an explicit batch of states that does not live in a handle --
 * selectActionBatch(number_of_actions, epsilon, grid_shift, toric_size, state, model, device)
 * (numba/util_actor.py:11-53) after the model forward.  The reference draws from numpy's global,
 * never seeded RNG (:49, :97-98); here the draw of state i is Philox keyed (seed, first_id + i,
 * call_counter) in its own domain, so the caller supplies a seed and a counter it advances per call. */
int tq_states_select_action(int n, const float* q_table, const int64_t* offsets,
                            const int32_t* positions, const double* eps, uint64_t seed,
                            uint64_t call_counter, int64_t first_id, int32_t* actions,
                            float* q_values, void* stream);

/* Reads and clears the calling device's error latch of the tq_states_* entry points (synchronises
 * `stream`): 0, TQ_E_ACTION, TQ_E_CAPACITY or TQ_E_INVALID (offsets that do not belong to the states). */
int tq_states_check(void* stream);

/* predictMaxOptimized's reduction (util_learner.py:96-110): out[i] = max over the (n_i,3) slice of
 * q_table, 0 for states without perspectives; `largest` = device i32[1] holding the longest slice
 * length reproduces the reference's zero padding (shorter slices get max(max_q, 0)); NULL = plain max. */
int tq_segment_max(const float* q_table, const int64_t* offsets, int n, const int32_t* largest,
                   float* out, void* stream);

/* The learner's TD targets behind the forward of the next states' perspectives (Learner_mp.py:146-151) in one launch:
 *   y[i] = clamp(rewards[i] + (terminals[i] ? 0 : 1) * discount * m[i], lo, hi)
 * with m[i] = tq_segment_max's result WITH the reference's zero padding: 0 for an empty slice, max(max_q, 0) for a slice
 * shorter than the batch's longest, max_q for one as long.  The longest slice is found on the device inside the call (no
 * `largest` argument, no host read).  q_table f32[P,3] (may be NULL when P = 0), offsets i64[n+1], rewards f32[n],
 * terminals u8[n] (0/1, a torch.bool tensor) -> y f32[n].  f32 arithmetic with the roundings of the torch expression
 * reward + (~terminal).float() * discount * target -- ((1 - t) * discount) * m, then + reward, then the clamp, nothing
 * contracted -- so y is bit-identical to that expression on the same inputs.
 * Non-finite values -- targets (tq_segment_max, tq_td_target, and max_a of tq_block_priorities alike).  A maximum is
 * np.amax: NaN if any element of the slice is NaN, else the largest, +-inf included.  The zero padding of a shorter slice
 * keeps a NaN a NaN (and turns -inf into 0, as max(-inf, 0) is).  The target expression is plain IEEE: 0 x NaN and 0 x inf
 * under a set terminal flag are NaN, as in torch, and the clamp passes NaN.  So a NaN Q-value of the target network gives a
 * NaN y (and a NaN priority) and never a finite number.  Out of scope: a NaN priority saved into the replay memory's sum
 * tree (tq_replay_save_block, tq_replay_update) -- the reference's tree breaks there as well. */
int tq_td_target(const float* q_table, const int64_t* offsets, int n, const float* rewards,
                 const uint8_t* terminals, float discount, float lo, float hi, float* y, void* stream);

/* generateTransitionParallel (util_actor.py:223-264) for the last tq_step: perspective of the
 * pre-step and post-step syndrome centred on the acted qubit (rotated for layer 1), action
 * rewritten to (layer, gs, gs, op).  Outputs (any may be NULL): persp u8[N,2,d,d],
 * next_persp u8[N,2,d,d], actions_out i32[N,4]. */
int tq_transition_write(tq_env* h, const int32_t* actions, uint8_t* persp, uint8_t* next_persp,
                        int32_t* actions_out, void* stream);

/* generateTransitionParallel(action, reward, state, next_state, terminal, grid_shift, type)
 * (util_actor.py:223-264) for explicit syndrome arrays that do not live in a handle:
 * states / next_states = device u8[n,2,d,d], actions = device i32[n,4]
 * -> persp u8[n,2,d,d], next_persp u8[n,2,d,d], actions_out i32[n,4] (any may be NULL). */
int tq_states_transition(int d, int n, const uint8_t* states, const uint8_t* next_states,
                         const int32_t* actions, uint8_t* persp, uint8_t* next_persp,
                         int32_t* actions_out, void* stream);

/* Packed transition block (the wire format gathered to the replay memory -- the (transition,
 * priority) pairs of Actor_mp.py:152, IO_mp.py:60-66): for `cap` transitions, SoA sections in this
 * order, each 8-byte aligned:
 *   persp_v u64[W][cap] | persp_p u64[W][cap] | next_v u64[W][cap] | next_p u64[W][cap] |
 *   action u32[cap] (layer | row<<8 | col<<16 | op<<24) | reward f32[cap] | priority f32[cap] |
 *   terminal u8[cap]
 * with W = ceil(d*d/64) and bit r*d+c of a plane = cell (r,c); 45 bytes per transition at d=7.
 * A slot whose action word is 0 (op = 0) holds no transition (the lattice was given a no-op or a
 * rejected action): all its other fields are zero and consumers drop it. */
int64_t tq_transition_block_bytes(int d, int64_t cap);
/* unpack slots [first, first+count) of a block into u8 grids / i32 actions (op 0 = empty slot) /
 * f32 rewards / u8 terminals / f32 priorities (any output may be NULL). */
int tq_transition_unpack(int d, const void* block, int64_t cap, int64_t first, int64_t count,
                         uint8_t* persp, uint8_t* next_persp, int32_t* actions, float* rewards,
                         uint8_t* terminals, float* priorities, void* stream);
/* computePrioritiesParallel (util_actor.py:268-287) into the block's priority section, for a block
 * that holds n_steps steps of n_envs lattices in slot order t*n_envs + e (what tq_actor_step writes):
 *   priority = | reward + discount * max_a Q[t+1][e][a] - Q[t][e][op-1] |   (f64 arithmetic, stored f32)
 * q_values = device f32[n_steps+1][n_envs][3]: the q_values selectActionBatch returned at each of the
 * n_steps steps plus the step after (local_buffer_Q and its np.roll(-1), Actor_mp.py:146-150);
 * NULL = all zeros (pure exploration).  Empty slots get priority 0.
 * Width: the reference's priorities are float64 (util_actor.py:287); the wire field is float32 -- the one
 * field of the record that is narrower than upstream.  The arithmetic is f64 and rounded once, so the
 * stored value is exactly float32(reference priority); a sum tree that needs f64 widens it on ingest. */
int tq_block_priorities(int d, void* block, int64_t cap, int n_envs, int n_steps,
                        const float* q_values, double discount, void* stream);

/* One fused iteration of the actor loop body after the policy (Actor_mp.py:116-183):
 *   step (EnvSet.step) -> transition record (generateTransitionParallel) -> reset of terminal
 *   / timed-out lattices with the p_error schedule (resetTerminalEnvs) -> perspective counts
 *   of the resulting states.
 * actions: device i32[N,4] from tq_select_action / the caller, or NULL = pure exploration
 * (eps = 1: uniform random perspective and op drawn in-kernel with the same Philox draws as
 * tq_select_action).  Outputs (may be NULL): actions_out i32[N,4] (the actions taken),
 * rewards f32[N], terminals u8[N], block/slot: packed transition block with capacity
 * `block_cap` transitions, lattice e writing slot `slot_base + e` (always: an empty slot when it
 * was given a no-op or a rejected action; the priority section is left to tq_block_priorities).
 *
 * Two streams: the step reads the lattices from one buffer of the handle and writes the other (the two take turns),
 * and tq_persp_count keeps two cut-point tables in turn.  So with actions == NULL (the selection does not look at the
 * stack) the caller may enqueue tq_actor_step(t) and tq_persp_count(t+1, into a SECOND offsets array) on another stream
 * than tq_persp_write(t): they run beside the stack write instead of behind it.  The caller orders what the handle
 * cannot see: tq_persp_write(t) behind tq_persp_count(t); tq_actor_step(t+1) behind tq_persp_write(t) (it overwrites
 * the buffer that write reads).  On one stream nothing changes.  The set-up and in-place entry points (reset, step,
 * set_qubits, getters) work on the current buffer in stream order like before. */
int tq_actor_step(tq_env* h, const int32_t* actions, int32_t* actions_out, float* rewards,
                  uint8_t* terminals, void* block, int64_t block_cap, int64_t slot_base,
                  void* stream);

/* Reads and clears the handle's device error latch (synchronises `stream`): 0, TQ_E_ACTION,
 * TQ_E_CAPACITY, TQ_E_INDEX, TQ_E_RESET or TQ_E_INVALID (offsets handed to tq_persp_write that are not the scan of the
 * lattices' counts, or a tq_select_action_planned whose plan was made with another eps or before a step). */
int tq_check(tq_env* h, void* stream);

/* ---- Prioritized replay memory on the device (PrioritizedReplayMemory / SumTree, src/ReplayMemory.py:45-152,
 * src/SumTree.py).  Records are kept in the wire format above (a packed SoA ring with the block's sections minus the
 * priority section); the priorities live in an f64 sum tree of the reference's shape: L = ceil(log2(capacity+1)) + 1
 * levels (computed as math.log(capacity+1, 2) is), heap order, leaf i = record i.  Between calls every internal node
 * is fl(left + right) -- the tree is a function of its leaves (no floating atomics).  Design: DESIGN.md §3.5.
 *  - one handle, one stream: the calls of a handle share its scratch and device state; issue them on one stream, or
 *    separate them by a synchronisation.  Capture of these calls into a HIP graph is not supported.
 *  - set-up calls (create, destroy) allocate and synchronise; so does the first tq_replay_save_block of a block larger
 *    than any before (its compaction scratch grows).  tq_replay_filled, tq_replay_check synchronise `stream`;
 *    everything else only enqueues kernels.
 *  - indices are int64 record indices (leaf numbers); uniforms / priorities / weights / tree values are f64.
 *  - errors seen on the device are latched and reported by tq_replay_check: TQ_E_CAPACITY (a sample of more records
 *    than are filled), TQ_E_INDEX (an index outside [0, filled), or a draw that ended on an unfilled leaf), and what the
 *    stack writer of tq_replay_next_persp_write latches: TQ_E_CAPACITY (stack capacity exceeded), TQ_E_INVALID (offsets
 *    that are not the scan of these records' counts).  Nothing outside the filled records is ever read. */
typedef struct tq_replay tq_replay;

/* PrioritizedReplayMemory(memory_size = capacity, alpha) for records of lattice size d; capacity 1..2^26, alpha >= 0.
 * seed keys the handle's own uniforms (RNG domain 5).  faithful = 1 keeps the reference's two exponent
 * quirks (sample's revert and reset_alpha), 0 drops them. */
int tq_replay_create(tq_replay** out, int d, int64_t capacity, double alpha, int device, uint64_t seed, int faithful);
int tq_replay_destroy(tq_replay* r);
/* replay_memory.save(t, p) for every transition of a packed block of `cap` slots (IO_mp.py:60-66): the non-empty slots
 * (action word != 0) in slot order, record k to ring position (cursor + k) % capacity; leaf = pow((double)priority,
 * alpha); of a block with more records than the capacity only the last `capacity` survive.  block: 8-byte aligned. */
int tq_replay_save_block(tq_replay* r, const void* block, int64_t cap, void* stream);
/* tree.filled_size(): number of records held (synchronises `stream`); < 0 on error. */
int64_t tq_replay_filled(tq_replay* r, void* stream);
/* PrioritizedReplayMemory.sample(batch, beta) (ReplayMemory.py:85-124), batch 1..4096: indices, priorities (the picked
 * leaf values) and normalised weights f64[batch] (required), and the picked records through the outputs of
 * tq_replay_get (any may be NULL).  uniforms: device f64[batch] in [0,1), or NULL = the handle's Philox stream.  With
 * faithful = 1 every picked leaf is then set to pow(leaf, alpha), last pick wins (the reference's "revert").  Weights
 * that are all 0 come back as 0 (the reference raises ZeroDivisionError there). */
int tq_replay_sample(tq_replay* r, int batch, double beta, const double* uniforms, int64_t* indices, double* priorities,
                     double* weights, float* state, float* next_state, int64_t* actions_idx, float* rewards,
                     uint8_t* terminals, int32_t* actions, void* stream);
/* records at indices[0..n) -> dataToBatch's tensors (util_learner.py:7-46): state / next_state f32[n,2,d,d],
 * actions_idx i64[n] (op - 1), rewards f32[n], terminals u8[n] (0/1), and the raw actions i32[n,4]. */
int tq_replay_get(tq_replay* r, const int64_t* indices, int n, float* state, float* next_state, int64_t* actions_idx,
                  float* rewards, uint8_t* terminals, int32_t* actions, void* stream);
/* The learner's target side straight from the ring (predictMaxOptimized's generatePerspectiveBatch on the batch's
 * next_state, util_learner.py:48-111, without expanding the records first): the two steps of tq_states_persp_count /
 * tq_states_persp_write for the NEXT-state syndromes of the records at indices[0..n), n in 1..4096, whose packed planes
 * are what the stack writer reads.  counts i32[n] (may be NULL), offsets i64[n+1]; then out[P,2,d,d] of `dtype`,
 * positions i32[P,3] (may be NULL), capacity in perspectives; alignment as for tq_persp_write.  A count depends on the
 * syndrome alone: a record with an empty next syndrome counts 0 whatever its terminal byte says.  An index outside
 * [0, filled) reads nothing, counts 0 and latches TQ_E_INDEX.  The write gathers the planes again, so a count / write
 * pair shares nothing but the handle's scratch (sized for 4096 records by tq_replay_create: no reserve call, no
 * allocation here), and it checks `offsets` on the device as tq_persp_write does: offsets that are not the scan of these
 * records' counts are refused (nothing stored outside [0, min(P, capacity)) perspectives, TQ_E_INVALID latched); lattices
 * that would overflow `capacity` are skipped and TQ_E_CAPACITY is latched (tq_replay_check reports both). */
int tq_replay_next_persp_count(tq_replay* r, const int64_t* indices, int n, int32_t* counts, int64_t* offsets,
                               void* stream);
int tq_replay_next_persp_write(tq_replay* r, const int64_t* indices, int n, const int64_t* offsets, void* out,
                               int32_t* positions, int64_t capacity, int dtype, void* stream);
/* priority_update(indices, priorities) (ReplayMemory.py:126-133): leaf = pow(p, alpha); of an index listed twice the
 * last occurrence wins. */
int tq_replay_update(tq_replay* r, const int64_t* indices, const double* priorities, int n, void* stream);
/* reset_alpha(alpha) (ReplayMemory.py:135-145) over the filled leaves; a zero leaf stays 0. */
int tq_replay_reset_alpha(tq_replay* r, double alpha, void* stream);
/* read-backs for tests: the leaves f64[capacity], the whole tree f64[tq_replay_tree_nodes(r)] (device buffers). */
int tq_replay_leaves(tq_replay* r, double* out, void* stream);
int64_t tq_replay_tree_nodes(const tq_replay* r);
int tq_replay_tree(tq_replay* r, double* out, void* stream);
/* Reads and clears the handle's device error latch (synchronises `stream`). */
int tq_replay_check(tq_replay* r, void* stream);

/* ---- The Q-network NN_11's forward pass on the device (src/nn/torch/NN.py:10-45: eleven conv3x3 + ReLU with channels
 * 2-128-128-120-111-104-103-90-80-73-71-64 and one linear layer to 3 outputs; src/nn/torch/util.py:21-26: the circular pad
 * of 1 before the unpadded conv1; zero padding 1 in conv2..10, conv11 unpadded).  It reads the perspective stack
 * tq_persp_write produces, in any of its four element types, and writes the (P,3) f32 Q-table that tq_select_action,
 * tq_segment_max and tq_td_target consume.  Design: DESIGN.md 3.6.
 * Numerics contract:
 *  - conv and linear weights are rounded once to bf16 (round to nearest even) when they are loaded; all biases stay f32.
 *  - a stack element is converted to bf16 (exact for the 0/1 the writer produces).
 *  - each conv layer accumulates bf16 x bf16 products in f32 (MFMA), adds the f32 bias, applies ReLU in f32 and rounds to
 *    bf16 (RNE) as the next layer's input; conv11's output is rounded the same way.
 *  - the linear layer accumulates in f32, adds the f32 bias and stores f32: Q-values are never rounded to 16 bits.
 *  - no atomics: the same call on the same inputs gives bit-identical output.
 *  - channels are padded with zero weights and biases up to the MFMA granule (32), so a padded activation channel is 0
 *    (on finite data: see "Non-finite values").
 * Non-finite values -- forward (NN_11, the wide nets and the ResNets alike).  A NaN in any input of a sum gives a NaN in
 * every output that depends on it, as the torch expression of the same operation does; NaNs are compared by position
 * only, their payload and sign are unspecified.  relu(NaN) = NaN, relu(+-0) = +0, relu(+inf) = +inf, relu(-inf) = +0.
 * bf16(x) is RNE for every finite x, +-inf for |x| at or beyond the rounding boundary (0x7f7f8000), and a NaN for every
 * NaN -- also for those whose low half would carry out of the exponent (0x7fffffff, 0xffffffff, 0x7f800001).  The zero
 * padding of a conv and the zero weights of a padded channel multiply like any other 0: 0 x inf and 0 x NaN are NaN, as in
 * torch, so an inf weight makes its output channel NaN where the activation it meets is 0, the padding included.  Rows
 * never meet: a non-finite stack element changes no other row's Q-values, and what a call leaves in the handle's scratch
 * changes no later call.  Finite inputs give the bits they gave before these rules were written down.
 * One handle, one stream: the calls of a handle share its packed weights and activation scratch; issue them on one
 * stream, or separate them by a synchronisation.  create / destroy are set-up calls (allocate, synchronise, leave the
 * caller's device unchanged); load and forward only enqueue kernels. */
typedef struct tq_nn11 tq_nn11;
/* NN_11(system_size = d, number_of_actions = 3) (NN.py:10-24) for passes of up to max_rows perspectives: allocates the
 * packed weights and two activation images of max_rows * d*d * 128 bf16.  Checked before the device is touched: out NULL,
 * d even or unsupported, max_rows <= 0 -> TQ_E_INVALID. */
int tq_nn11_create(tq_nn11** out, int d, int64_t max_rows, int device);
int tq_nn11_destroy(tq_nn11* h);
/* model.load_state_dict (NN.py:10-24): weights[12] / biases[12] are HOST arrays of device pointers to f32 tensors in torch
 * layout -- conv1..conv11 weight [cout][cin][3][3] and bias [cout], then linear1 weight [3][64*(d-2)^2] (features in
 * (channel, y, x) order) and bias [3].  Packs on the device; cheap enough for a weight refresh at every flush. */
int tq_nn11_load(tq_nn11* h, const float* const* weights, const float* const* biases, void* stream);
/* model(stack) (NN.py:26-45, util.py:21-26): stack[rows][2][d][d] of element type dtype (TQ_F32 / TQ_F16 / TQ_BF16 /
 * TQ_U8, 16-byte aligned) -> q f32[rows][3].  Any rows >= 0: the call walks passes of max_rows itself.  TQ_E_INVALID
 * before the first tq_nn11_load. */
int tq_nn11_forward(tq_nn11* h, const void* stack, int dtype, int64_t rows, float* q, void* stream);
/* model(stack[rows]): q[i] = the Q-values of perspective rows[i] of stack[stack_rows][2][d][d], i < n, read in place by
 * conv1 -- the same bits as tq_nn11_forward's q[rows[i]].  rows: device i32[n], any list: unsorted, with repeats.  Any
 * n >= 0 (passes of max_rows, like tq_nn11_forward); the same arguments are refused before any launch, and a NULL rows
 * or negative stack_rows.  An index outside [0, stack_rows) reads nothing: its q row is that of an all-zero perspective,
 * every other row is unaffected, and TQ_E_INDEX is latched for tq_nn11_check. */
int tq_nn11_forward_rows(tq_nn11* h, const void* stack, int dtype, int64_t stack_rows, const int32_t* rows,
                         int64_t n, float* q, void* stream);
/* Reads and clears the forward handle's device error latch (synchronises `stream`): 0 or TQ_E_INDEX. */
int tq_nn11_check(tq_nn11* h, void* stream);

/* ---- NN_11's learner step (src/Learner_mp.py:140-169): the forward with every layer's output kept, the gather of
 * Q(s,a), the weighted squared error, the backward pass and the parameter gradients.  The optimizer works on the caller's
 * f32 master parameters: the caller's own, or tq_nn11_grad_opt_step below.  Design: DESIGN.md 3.7.
 * Numerics contract.  The forward is tq_nn11_forward's: A_0 is the stack converted to bf16, A_l (l = 1..11) the layers'
 * bf16 outputs, q is f32 and bit-equal to tq_nn11_forward on the same weights and rows.
 *  Head, per record i with a = actions_idx[i], all in f32, each operation rounded once, left to right, nothing contracted:
 *   - e = y[i] - q[i][a];  loss[i] = w[i] * (e * e)  (the reference takes |loss[i]| as the record's new priority);
 *   - dq[i][a] = (((q[i][a] - y[i]) * w[i]) * 2) / (float)n, the row's other two entries 0: the gradient of
 *     mean_i(loss[i]) (Learner_mp.py:152-160);  w == NULL means all ones;
 *   - actions_idx[i] outside 0..2: loss[i] = 0, dq[i] = 0, and TQ_E_ACTION is latched (tq_nn11_grad_check).
 *  Gradients of the pre-activations, G_l for layer l, stored as bf16 (RNE; bf16 has f32's exponent range: no loss scaling):
 *   - the ReLU mask is A_l > 0 on the stored bf16 activation, and a NaN activation lets the gradient through: the mask
 *     blocks where A_l <= 0 (torch's threshold_backward);
 *   - G_11 = bf16(mask_11 * sum_a dq[.][a] * Wlin_bf16[a][.]);
 *   - l = 11..2: G_{l-1} = bf16(mask_{l-1} * conv_transpose(G_l, W_l rounded to bf16)), accumulated in f32; conv11 is
 *     unpadded, so its transpose is a full correlation from the (d-2)^2 grid onto the d^2 grid;
 *   - no gradient is formed for the stack.
 *  Parameter gradients, f32 in torch layout, written (not accumulated):
 *   - dW_l[co][ci][ky][kx] = sum over records and pixels of G_l * A_{l-1}(shifted by the tap; conv1: with the circular
 *     wrap), bf16 x bf16 products accumulated in f32;  db_l = sum G_l;
 *   - dWlin = dq^T A_11 in torch's (channel, y, x) feature order;  dblin = sum_i dq[i];
 *   - these are gradients at the bf16-rounded weights, to be applied to the f32 masters (straight-through).
 *  Determinism: no atomics in any sum; how a sum is cut into partial sums depends on (d, n) alone, never on occupancy or
 *  timing: the same call gives the same bits.  A padded channel's G is 0 because its mask is 0.
 *  Non-finite values -- learner step.  The forward's rules hold for A_l and q.  The head is plain IEEE: a NaN y, an inf w
 *  or a NaN q[i][a] gives record i a non-finite loss[i] and dq[i][a] and leaves loss and q of every other record unchanged
 *  in bits.  Every sum of the backward (G_l, dW_l, db_l, dWlin, dblin) propagates like the forward's, the bf16 of a G as
 *  above: a gradient element is NaN where the f32 autograd of this contract makes it one.  A step full of NaN leaves
 *  nothing in the handle's scratch that a later step reads.
 * One handle, one stream, as for tq_nn11_*: create / destroy allocate and synchronise, load and step only enqueue. */
typedef struct tq_nn11_grad tq_nn11_grad;
/* Allocates both weight images, the eleven activation images (each of its layer's own padded channel count), two gradient
 * images and the wgrad partial images for steps of up to max_batch (1..4096) records. */
int tq_nn11_grad_create(tq_nn11_grad** out, int d, int max_batch, int device);
int tq_nn11_grad_destroy(tq_nn11_grad* h);
/* weights / biases as for tq_nn11_load; packs the forward and the dgrad images on the device. */
int tq_nn11_grad_load(tq_nn11_grad* h, const float* const* weights, const float* const* biases, void* stream);
/* One step on state[n][2][d][d] (element type dtype, 16-byte aligned): actions_idx i64[n] in 0..2, y f32[n], w f32[n] or
 * NULL -> q f32[n][3] (may be NULL), loss f32[n], and the gradients into grad_w[12] / grad_b[12], HOST arrays of device
 * pointers to f32 tensors in the layout of tq_nn11_load's.  Checked before any launch (TQ_E_INVALID): n outside
 * 1..max_batch, a NULL pointer, a misaligned state, a call before the first load. */
int tq_nn11_grad_step(tq_nn11_grad* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y,
                      const float* w, float* q, float* loss, float* const* grad_w, float* const* grad_b, void* stream);
/* Reads and clears the handle's device error latch (synchronises `stream`): 0 or TQ_E_ACTION. */
int tq_nn11_grad_check(tq_nn11_grad* h, void* stream);

/* ---- NN_11's optimizer step (src/Learner_mp.py:81-84: Adam or RMSprop on the f32 masters) in one launch: reads the
 * gradients tq_nn11_grad_step wrote, updates the masters and the optimizer state in place and, from the same registers,
 * rewrites the handle's bf16 forward image, dgrad image, biases and linear image, so that no tq_nn11_grad_load follows.
 * Design: DESIGN.md 3.8.
 * Numerics contract.  Per element, all in f32, each operation rounded once in the order the parentheses give, nothing
 * contracted; sqrt and / are IEEE correctly rounded (hipcc's default for f32, which the contract relies on) and subnormals
 * are kept.  NaN and Inf propagate as IEEE has it; nothing is clamped: a NaN or inf gradient element makes p' a NaN, and
 * the element's place in every image one (bf16 as in the forward's contract: a NaN stays a NaN).
 *  Scalars: computed on the host in double as Python does (b^t is pow), each cast to f32 once; t = step, the 1-based count
 *  of this update.
 *  TQ_OPT_ADAM:  c1 = (float)(1 - beta1), c2 = (float)beta2, c3 = (float)(1 - beta2), cb = (float)sqrt(1 - beta2^t),
 *   ce = (float)eps, cs = (float)(-(lr / (1 - beta1^t)))
 *   - m' = m + c1 * (g - m)
 *   - v' = (v * c2) + ((c3 * g) * g)
 *   - den = (sqrt(v') / cb) + ce
 *   - p' = p + cs * (m' / den)
 *  TQ_OPT_RMSPROP (momentum 0, not centered):  ca = (float)alpha, c3 = (float)(1 - alpha), ce, cs = (float)(-lr)
 *   - s' = (s * ca) + ((c3 * g) * g)
 *   - p' = p + cs * (g / (sqrt(s') + ce))
 *  These are the expressions of torch's single-tensor Adam and RMSprop with weight_decay 0, no amsgrad, no maximize.  They
 *  are not bit-equal to torch, which has no single answer in bits itself (its loops are vectorised and fused differently
 *  per backend); the lines above are the definition, torch is an accuracy reference.
 *  Images: bf16(p') (round to nearest even) goes to the element's place in the forward image and, for conv2..conv11, in
 *  the dgrad image; the linear layer's image gets that bf16 value as f32; biases go in as f32.  After the call the images
 *  are bit for bit what tq_nn11_grad_load would pack from the updated masters.  No atomics; the same call gives the same
 *  bits.
 * Every pointer argument is a HOST array of 12 device pointers in tq_nn11_load's order and layouts.  The caller owns the
 * state tensors as it owns the masters and the gradients (zero them before step 1); the handle keeps no optimizer state
 * and no step count.  m_w / m_b: Adam's exp_avg, not read for TQ_OPT_RMSPROP (may be NULL); v_w / v_b: Adam's exp_avg_sq
 * or RMSprop's square_avg.  Tensors whose pointers are all 16-byte aligned are accessed with 16-byte loads and stores.
 * Checked before the launch (TQ_E_INVALID): a NULL handle or one that was never loaded; a kind that is neither; lr < 0,
 * eps < 0, a beta (Adam) or alpha (RMSprop) outside [0, 1), any NaN among them; step < 1; a NULL pointer that the kind
 * needs.  Weight decay, amsgrad, momentum, centered and maximize are outside the contract and have no argument.
 * Precondition: the handle's images were packed from these masters, by tq_nn11_grad_load or an earlier
 * tq_nn11_grad_opt_step.  The call allocates nothing and does not synchronise. */
#define TQ_OPT_ADAM 0
#define TQ_OPT_RMSPROP 1
int tq_nn11_grad_opt_step(tq_nn11_grad* h, int kind, double lr, double beta1, double beta2, double eps, double alpha,
                          int64_t step, float* const* weights, float* const* biases, const float* const* grad_w,
                          const float* const* grad_b, float* const* m_w, float* const* m_b, float* const* v_w,
                          float* const* v_b, void* stream);

/* ---- The forward pass of the reference's two wide Q-networks on the device (src/nn/torch/NN.py:47-133):
 *   TQ_NET_NN8   NN_8:  8 conv3x3 + ReLU, channels 2-256-256-240-224-220-215-205-200
 *   TQ_NET_NN17  NN_17: 20 conv3x3 + ReLU despite its name, channels 2-256-256-251-250-240-240-235-233-233-229-225-223-
 *                220-220-220-215-214-205-204-200
 * each with NN_11's paddings (circular pad of 1 before the unpadded first conv, zero padding 1 in the middle convs, the
 * last conv unpadded) and one linear layer from 200 * (d-2)^2 features to 3 outputs.  Same stacks in, same (P,3) f32
 * Q-table out as tq_nn11_forward.  Their learner step is tq_nnw_grad_* below; the optimizer stays with the caller.  Design:
 * DESIGN.md 3.10.
 * Numerics contract -- NN_11's:
 *  - conv and linear weights are rounded once to bf16 (round to nearest even) when they are loaded; all biases stay f32.
 *  - a stack element is converted to bf16 (exact for the 0/1 the writer produces).
 *  - each conv layer accumulates bf16 x bf16 products in f32 (MFMA), adds the f32 bias, applies ReLU in f32 and rounds to
 *    bf16 (RNE) as the next layer's input; the last conv's output is rounded the same way.
 *  - the linear layer accumulates in f32, adds the f32 bias and stores f32.
 *  - channels are padded with zero weights and biases up to the MFMA granule (32), so a padded activation channel is 0.
 *  - the order of every sum depends on (net, layer, d) alone; no atomics: the same call gives the same bits, and a row's
 *    bits do not depend on its place in the batch or on how the call is cut into passes.
 * One handle, one stream, as for tq_nn11_*: create / destroy allocate and synchronise, load and forward only enqueue. */
#define TQ_NET_NN8 8
#define TQ_NET_NN17 17
typedef struct tq_nnw tq_nnw;
/* NN_8 / NN_17(system_size = d, number_of_actions = 3) for passes of up to max_rows perspectives: allocates the packed
 * weights and two activation images of max_rows * d*d * 256 bf16.  Checked before the device is touched: out NULL, net
 * neither, d even or unsupported, max_rows outside 1..2^24 -> TQ_E_INVALID. */
int tq_nnw_create(tq_nnw** out, int net, int d, int64_t max_rows, int device);
int tq_nnw_destroy(tq_nnw* h);
/* model.load_state_dict: weights[L + 1] / biases[L + 1] (L = 8 or 20 conv layers) are HOST arrays of device pointers to
 * f32 tensors in torch layout -- conv1..convL weight [cout][cin][3][3] and bias [cout], then linear1 weight
 * [3][200*(d-2)^2] (features in (channel, y, x) order) and bias [3].  Packs on the device. */
int tq_nnw_load(tq_nnw* h, const float* const* weights, const float* const* biases, void* stream);
/* model(stack): stack[rows][2][d][d] of element type dtype (TQ_F32 / TQ_F16 / TQ_BF16 / TQ_U8, 16-byte aligned) -> q
 * f32[rows][3].  Any rows >= 0: the call walks passes of max_rows itself.  TQ_E_INVALID before the first tq_nnw_load. */
int tq_nnw_forward(tq_nnw* h, const void* stack, int dtype, int64_t rows, float* q, void* stream);

/* ---- The wide nets' learner step (src/Learner_mp.py:140-169): tq_nn11_grad_*'s for NN_8 and NN_17.  The optimizer works
 * on the caller's f32 master parameters (torch.optim; there is no optimizer kernel for these nets), and tq_nnw_grad_load
 * packs them again.  Design: DESIGN.md 3.12.
 * Numerics contract: that of NN_11's learner step above, word for word, with these substitutions:
 *   - the layers are l = 1..L, L = 8 (NN_8) or 20 (NN_17), over the channel lists of TQ_NET_NN8 / TQ_NET_NN17; A_L, G_L,
 *     mask_L and conv L stand where A_11, G_11, mask_11 and conv11 do;
 *   - the last conv is the unpadded one, so it is conv L's transpose that is the full correlation from the (d-2)^2 grid
 *     onto the d^2 grid;
 *   - the linear layer has 200 features per pixel (in a pitch of 224, the padding 0): dWlin is f32[3][200*(d-2)^2].
 *  What carries over unchanged: q is f32 and bit-equal to tq_nnw_forward on the same weights and rows; the head is NN_11's
 *  expression, each operation rounded once, left to right; G_l is stored as bf16 (RNE); the ReLU mask is A_l > 0 on the
 *  stored bf16 activation; every product is bf16 x bf16 and every sum f32; the parameter gradients are f32 in torch
 *  layout, written (not accumulated), gradients at the bf16-rounded weights; no gradient is formed for the stack; an
 *  actions_idx outside 0..2 gives loss 0, dq 0 and latches TQ_E_ACTION.
 *  Determinism: no atomics in any sum; how a sum is cut into partial sums depends on (net, layer, d, n) alone, never on
 *  occupancy or timing: the same call gives the same bits.
 * One handle, one stream, as for tq_nnw_*: create / destroy allocate and synchronise, load and step only enqueue. */
typedef struct tq_nnw_grad tq_nnw_grad;
/* net: TQ_NET_NN8 or TQ_NET_NN17.  Allocates both weight images, every layer's activation image (each of its layer's own
 * padded channel count), two gradient images of max_batch * d*d * 256 bf16 and the wgrad partial images (one of 9 * 256 *
 * 256 f32 per chunk of records; the chunk is a function of d alone) for steps of up to max_batch (1..4096) records.
 * Checked before the device is touched: out NULL, net neither, d even or unsupported, max_batch outside 1..4096. */
int tq_nnw_grad_create(tq_nnw_grad** out, int net, int d, int max_batch, int device);
int tq_nnw_grad_destroy(tq_nnw_grad* h);
/* weights / biases as for tq_nnw_load; packs the forward and the dgrad images on the device. */
int tq_nnw_grad_load(tq_nnw_grad* h, const float* const* weights, const float* const* biases, void* stream);
/* One step on state[n][2][d][d] (element type dtype, 16-byte aligned): actions_idx i64[n] in 0..2, y f32[n], w f32[n] or
 * NULL -> q f32[n][3] (may be NULL), loss f32[n], and the gradients into grad_w[L + 1] / grad_b[L + 1], HOST arrays of
 * device pointers to f32 tensors in the layout of tq_nnw_load's.  Checked before any launch (TQ_E_INVALID): n outside
 * 1..max_batch, a NULL pointer, a misaligned state, a call before the first load.  The call allocates nothing and does not
 * synchronise. */
int tq_nnw_grad_step(tq_nnw_grad* h, const void* state, int dtype, int n, const int64_t* actions_idx, const float* y,
                     const float* w, float* q, float* loss, float* const* grad_w, float* const* grad_b, void* stream);
/* Reads and clears the handle's device error latch (synchronises `stream`): 0 or TQ_E_ACTION. */
int tq_nnw_grad_check(tq_nnw_grad* h, void* stream);

/* ---- The forward pass of the reference's BasicBlock ResNets on the device (src/nn/torch/ResNet.py), forward only and
 * with BatchNorm in inference form only (running statistics: the network as model.eval() computes it):
 *   TQ_NET_RESNET18  ResNet(BasicBlock, [2,2,2,2]), the reference launcher's default model
 *   TQ_NET_RESNET34  ResNet(BasicBlock, [3,4,6,3]): the same layer shapes, other block counts
 * conv1 3x3 2 -> 64 (zero padding 1, no bias) + bn1 + ReLU; layer1..layer4 of BasicBlocks at 64 / 128 / 256 / 512
 * channels, relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x)), the shortcut being the identity or, in the first block of
 * layer2..layer4, conv1x1 + bn; layer4's first block has stride 2, so for lattice size d the pixel grid is d x d up to
 * layer3 and s x s, s = (d+1)/2, from there on: the 3x3 of stride 2 reads source pixel (2y+ky-1, 2x+kx-1), zero outside
 * the grid, the 1x1 of stride 2 reads (2y, 2x); then the average over the s^2 pixels and Linear(512, 3).  Same stacks in,
 * same (P,3) f32 Q-table out as tq_nn11_forward.  A training-mode forward (batch statistics), the learner step and the
 * optimizer stay with the caller.  Design: DESIGN.md 3.11.
 * Numerics contract -- NN_11's extended.  All arithmetic is f32, every operation rounded once, nothing contracted; sqrt and
 * / are IEEE correctly rounded:
 *  - a stack element is converted to bf16 (exact for 0/1); conv weights are rounded once to bf16 (RNE), unscaled, when
 *    they are loaded; every convolution is a sum of bf16 x bf16 products in f32 (MFMA).
 *  - BatchNorm is folded at load into two f32 vectors per convolution: scale s = gamma / sqrt(running_var + eps), shift
 *    t = beta - running_mean * s (eps as f32); padding channels get s = 0 and t = 0, so a padded activation channel is 0.
 *  - epilogue of a convolution: z = acc * s + t; for a block's second convolution z = z + r, r being the f32 value of the
 *    shortcut's bf16 element (the block's input image, or the shortcut convolution's image); then ReLU; then ONE rounding
 *    to bf16 (RNE).
 *  - a shortcut convolution writes bf16(acc * s + t), without ReLU.  This rounding point has no counterpart in torch,
 *    where the shortcut's f32 value is added unrounded.
 *  - head: S[c] is the f32 sum of channel c over the s^2 pixels in pixel order; Q[a] = (sum_c S[c] * bf16(W[a][c])) / s^2
 *    + b[a], the sum over c in a fixed order (a lane's eight channels in order, then a butterfly over the 64 lanes).
 *    Dividing after the linear sum is mathematically torch's mean-then-linear and keeps every intermediate an integer on
 *    integer networks, so the head is exact there at every size, not only where s^2 is a power of two.
 *  - the order of every sum is (chunk, tap, k-step) and depends on (net, convolution, d) alone; no atomics: the same call
 *    gives the same bits, and a row's bits do not depend on its place in the batch, on the row count or on how the call is
 *    cut into passes.
 * One handle, one stream, as for tq_nn11_*: create / destroy allocate and synchronise, load and forward only enqueue. */
#define TQ_NET_RESNET18 18
#define TQ_NET_RESNET34 34
typedef struct tq_resnet tq_resnet;
/* ResNet18 / ResNet34 at lattice size d for passes of up to max_rows perspectives: allocates the packed weights and four
 * activation images of max_rows * d*d * 256 bf16 (a block's input, mid image, shortcut image and output are live at once;
 * 512 s^2 <= 256 d^2 for every supported d).  The weights do not depend on d.  Checked before the device is touched: out
 * NULL, net neither, d even or unsupported, max_rows outside 1..2^24 -> TQ_E_INVALID. */
int tq_resnet_create(tq_resnet** out, int net, int d, int64_t max_rows, int device);
int tq_resnet_destroy(tq_resnet* h);
/* model.load_state_dict: conv_weights[n] and bn_params[4 n] (n = 20 or 36 convolutions) are HOST arrays of device
 * pointers to f32 tensors in torch layout, in the order of the module's state_dict -- conv1, then per block conv1, conv2
 * and, where the block has one, shortcut.0: weight [cout][cin][3][3] or [cout][cin][1][1]; bn_params[4 i ..] are
 * convolution i's BatchNorm weight (gamma), bias (beta), running_mean and running_var, [cout] each.  lin_w: linear.weight
 * [3][512], lin_b: linear.bias [3], device pointers.  eps: the BatchNorm layers' eps, > 0.  Packs and folds on the device. */
int tq_resnet_load(tq_resnet* h, const float* const* conv_weights, const float* const* bn_params, const float* lin_w,
                   const float* lin_b, double eps, void* stream);
/* model.eval()(stack): stack[rows][2][d][d] of element type dtype (TQ_F32 / TQ_F16 / TQ_BF16 / TQ_U8, 16-byte aligned) ->
 * q f32[rows][3].  Any rows >= 0: the call walks passes of max_rows itself.  TQ_E_INVALID before the first
 * tq_resnet_load. */
int tq_resnet_forward(tq_resnet* h, const void* stack, int dtype, int64_t rows, float* q, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TORICENV_H */
