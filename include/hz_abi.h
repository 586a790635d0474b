/* hz_abi.h — C-ABI of libhz.so, the MI355X-native Harmonies self-play engine.
 *
 * The reference (IllyaArtemchuk/Harmonies-Alphazero) is pure Python with no
 * FFI; its hot path is reached through duck-typed Python surfaces.  Each entry
 * point below is the batched device form of one of those surfaces (cited as
 * /root/reference file:line).  The Python package
 * harmonies-alphazero_amd/hzamd binds them with ctypes; INTEGRATION.md shows
 * the binding a maintainer would add.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer (e.g. torch tensor.data_ptr())
 *    unless stated otherwise; it must stay valid until the work enqueued on
 *    the handle's stream has run.  Calls are asynchronous, stream-ordered on
 *    the handle's stream, and never allocate or synchronize.
 *  - Return value: 0 = enqueued; <0 = invalid argument (nothing enqueued);
 *    >0 = hipError_t of the failed launch.
 *  - Per-board rule violations are not errors of the call: they come back as
 *    per-board status codes (HZ_ST_*), where the reference raises ValueError.
 *  - Board b's state is the structure-of-arrays record documented in
 *    harmonies-alphazero_amd/csrc/hz_device.hpp (six u64 words, word w at
 *    state[w * n + b]); its chance stream is a CPython MT19937 (624 words at
 *    mt[b * 624 + i] plus a cursor).
 */
#ifndef HZ_ABI_H
#define HZ_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-board status codes (reference ValueError sites in parentheses) */
enum {
  HZ_ST_OK = 0,
  HZ_ST_BAD_PILE = 1,        /* harmonies_engine.py:216-220 "Invalid pile index"      */
  HZ_ST_BAD_FORMAT = 2,      /* :227-236 "Invalid move format for placement phase"     */
  HZ_ST_NOT_IN_HAND = 3,     /* :244-248 "Illegal move attempted: Tile ... not in hand" */
  HZ_ST_ILLEGAL_STACK = 4,   /* :281-283 "Cannot place ... on ... with stack"           */
  HZ_ST_BAD_PHASE = 5,       /* :296-297 "Invalid turn phase"                           */
  HZ_ST_BAD_ACTION = 6,      /* action id outside [0,143) (process_game_state.py:156-179) */
  HZ_ST_NOOP = 7             /* negative action: board left untouched                    */
};

typedef struct hz_env hz_env;

/* ---- lifecycle ---------------------------------------------------------- */
/* n_boards boards; board b's k-th game is seeded like
 * random.seed(seed_base + b + (k << 32)) followed by HarmoniesGameState()
 * (harmonies_engine.py:66-79).  stream: hipStream_t, NULL = null stream.
 * The handle owns all device buffers (48 B state + 2.5 KB MT per board). */
hz_env *hz_env_create(int32_t n_boards, uint64_t seed_base, void *stream);
void hz_env_destroy(hz_env *env);
int32_t hz_env_size(const hz_env *env);
int hz_env_set_stream(hz_env *env, void *stream);
/* device pointers of the handle's own buffers (for zero-copy views) */
uint64_t *hz_env_state_ptr(hz_env *env);     /* [6][n]            */
/* The two stream pointers are for a caller that may move or rewrite the
 * streams: each call first voids, in stream order, the draw words that
 * hz_step / hz_rule_ply keep per board between plies (one small fill). */
uint32_t *hz_env_mt_ptr(hz_env *env);        /* [n][624]          */
int32_t *hz_env_mt_pos_ptr(hz_env *env);     /* [n]               */
/* The same two pointers without that fill, for a kernel launched once per
 * simulation (hz_mcts_expand_backup*): the streams are made current, and the
 * caller's kernel must itself store -1 to win_tag[b] ([n], the board's saved
 * draw window: none) for every board b whose stream words or cursor it
 * writes, in the launch that writes them.  0 on success. */
int hz_env_stream_ptrs(hz_env *env, uint32_t **mt, int32_t **mt_pos, int32_t **win_tag);
int32_t *hz_env_ply_ptr(hz_env *env);        /* [n] plies played in the current game */
uint64_t *hz_env_seed_ptr(hz_env *env);      /* [n] seed of the current game */

/* ---- env surface (step / reset / legal_actions / score) ----------------- */
/* reset: HarmoniesGameState() for every board with sel[b] != 0 (sel NULL =
 * all boards).  seeds (optional, [n]) overrides the per-board seed. */
int hz_reset(hz_env *env, const uint8_t *sel, const uint64_t *seeds);

/* legal_actions: get_legal_moves (harmonies_engine.py:145-208) mapped through
 * get_action_index (process_game_state.py:156-179) to a 143-bit mask per
 * board, mask[b*3 + w] bit i = action 64*w + i.  count[b] = #legal (may be
 * NULL).  A finished board has an empty mask. */
int hz_legal_mask(hz_env *env, uint64_t *mask, int32_t *count);
/* the same legal moves as one byte per action: legal[b*143 + a] = 1 when
 * action a is legal on board b (a bool [n][143] tensor; legal 16-B aligned),
 * count as above.  One launch for BatchedEnv.legal_actions(). */
int hz_legal_actions(hz_env *env, uint8_t *legal, int32_t *count);

/* step: apply_move (harmonies_engine.py:210-298) in place, including
 * _end_turn_actions (:301-329) and chance draws.  action[b] < 0 = no-op.
 * status[b] (may be NULL) gets an HZ_ST_* code; on a non-zero status the
 * board is unchanged (the reference raises before committing its clone). */
int hz_step(hz_env *env, const int16_t *action, int32_t *status);

/* _replenish_piles (harmonies_engine.py:132-137) / _end_turn_actions
 * (:301-329) on the selected boards (sel NULL = all), drawing from each
 * board's stream.  The Python facade uses them for HarmoniesGameState() and
 * for callers that invoke _end_turn_actions directly (text_game.py:212). */
int hz_replenish(hz_env *env, const uint8_t *sel);
int hz_end_turn(hz_env *env, const uint8_t *sel);

/* score: calculate_score_for_player(p) (:357-367) for both players of every
 * board, out[b*2 + p].  parts (may be NULL): out_parts[(b*2+p)*5 + k] for
 * grass, mountains, fields, buildings, water (:369-523). */
int hz_score(hz_env *env, int32_t *out, int32_t *out_parts);

/* encode: create_state_tensors (process_game_state.py:15-137) for boards
 * idx[0..m) (idx NULL = boards 0..m-1): board[m][38][5][7], glob[m][42], f32. */
int hz_encode(hz_env *env, const int32_t *idx, int32_t m, float *board, float *glob);

/* Stateless encoder over any state array (replay records, tree nodes): item j
 * is idx[j] (idx NULL = j); its word w is states[item * item_stride +
 * w * word_stride].  idx[j] < 0 yields zeros.  Enqueued on `stream`. */
int hz_encode_states(const uint64_t *states, int64_t word_stride, int64_t item_stride, const int32_t *idx,
                     int32_t m, float *board, float *glob, void *stream);

/* ---- board symmetries ---------------------------------------------------- */
/* The 23-cell board has four automorphisms, and each is an automorphism of
 * the whole game: placement rules and all five scorers see only stacks and
 * adjacency; piles, hand, bag and the chance stream never see a coordinate.
 * Group element g in 0..3 maps an axial coordinate (tensor position x = q + 3,
 * y = r + 2):
 *   g = 0  (q, r)          (x, y)
 *   g = 1  (-q, -r)        (6 - x, 4 - y)          the half turn
 *   g = 2  (q + r, -r)     (x + y - 2, 4 - y)      a reflection
 *   g = 3  (-q - r, r)     (8 - x - y, y)          the other reflection
 * a after b is a ^ b (Klein four-group): every element is its own inverse.
 * With cells indexed as everywhere (c = index into sorted(VALID_HEXES)),
 * perm[g][c] is the index of the image of cell c:
 *   perm[1][c] = 22 - c
 *   perm[2] = 4 1 5 9 0 2 6 10 14 3 7 11 15 19 8 12 16 20 22 13 17 21 18
 *   perm[3][c] = 22 - perm[2][c]
 * State:  for both players the stack code at cell c moves to cell perm[g][c]:
 *         in each of the four plane words, bits 0..22 and bits 32..54 are
 *         permuted and every other bit is kept; piles and misc are untouched.
 * Action: a < 5 is unchanged; 5 + 23 t + c maps to 5 + 23 t + perm[g][c].
 * Record (42 int64: six state words | 143 u16 slots | int8 z | int8 player):
 *         the state words as above, the slots permuted by the action map
 *         (visit counts and quantised policies alike), z and player kept.
 * Both calls below are asynchronous on `stream`, allocate nothing and do not
 * synchronize; records need only their natural 8-byte alignment. */

/* out[j] = record rec[j] under symmetry sym[j] & 3 (sym NULL = identity, a plain copy).
 * out may equal rec (each record is read whole before it is written). m = 0 is a no-op.
 * <0: m < 0, or m > 0 with a NULL rec / out; nothing enqueued. */
int hz_sym_records(const int64_t *rec, int64_t m, const uint8_t *sym, int64_t *out, void *stream);

/* One training batch from packed records in one launch: item j is record idx[j]
 * (idx NULL = j; idx[j] < 0 yields zeros everywhere) under symmetry sym[j] & 3
 * (NULL = identity):
 *   board[m][38][5][7], glob[m][42]  = hz_encode_states of the transformed state,
 *   pi[m][143] = (float)((double)v[a] / (double)sum v), all zeros where the sum is 0
 *                (the bits of hzamd.distributed.pi_of),
 *   z[m]       = (float)(int8) z byte.
 * <0: m < 0 or a NULL output; nothing enqueued. */
int hz_train_batch(const int64_t *rec, const int32_t *idx, const uint8_t *sym, int32_t m,
                   float *board, float *glob, float *pi, float *z, void *stream);

/* Build-defined deterministic policy used by the env benchmark and the golden
 * traces: pick legal action k = ((splitmix64(seed, ply) >> 32) * L) >> 32 in
 * ascending action order.  Writes action[b] (-1 if no legal move). */
int hz_rule_actions(hz_env *env, const uint64_t *mask, const int32_t *count, int16_t *action);

/* One ply of the per-ply surface for every board in ONE launch:
 * get_legal_moves (harmonies_engine.py:145-208, as hz_legal_mask) -> the
 * rule pick above (as hz_rule_actions) -> apply_move (:210-298, as hz_step).
 * Each output pointer may be NULL; those given get exactly what the three
 * separate calls would write (mask, count, action, status).  The batched
 * API path's graph replays one of these per ply instead of three launches. */
int hz_rule_ply(hz_env *env, uint64_t *mask, int32_t *count, int16_t *action, int32_t *status);

/* evaluation.py:137-196 choose_move_greedy for every selected board (sel may
 * be NULL = all): the legal move whose resulting board scores highest for the
 * player to move, first strictly best in ascending action order.  Like the
 * reference, whose simulated apply_move calls refill the piles from the
 * global `random` at the end of a turn, it consumes each board's chance
 * stream once per candidate when the phase is place_tile_3; apply the
 * returned move with hz_step.  action[b] = -1 when unselected, finished or
 * without a legal move. */
int hz_greedy_actions(hz_env *env, const uint8_t *sel, int16_t *action);

/* Fused env loop: every board plays up to max_plies rule-driven plies
 * (legal mask -> rule pick -> step), stopping at game end (auto_reset = 0) or
 * starting its next game (auto_reset != 0).  Optional per-ply records
 * (NULL = off): traj_state[(ply*6 + w)*n + b], traj_mask[(ply*n + b)*3 + w],
 * traj_action[ply*n + b] (-1 after the game ended).  games_done[b] counts
 * games finished during the call, steps_done[b] env steps taken.
 * A stuck board (no legal move although the game is not over; no play from
 * hz_reset reaches one, hz_import_state can bring one in) is defined API
 * behaviour with no reference counterpart (MCTS.py only logs the case):
 * hz_rollout and hz_play stop such a board for the rest of the call, with
 * auto_reset on or off: no step and no game counted from there on, and its
 * state, stream, ply count, seed and episode stay as they are; the other
 * boards are not affected.  On the per-ply surface the same board gets an
 * empty mask and count 0 (hz_legal_mask, hz_legal_actions), action -1
 * (hz_rule_actions, hz_greedy_actions, neither drawing from its stream) and
 * HZ_ST_NOOP from hz_step / hz_rule_ply; a search leaves its root without
 * visits (hz_mcts_result all zero, 1 node, 0 edges). */
int hz_rollout(hz_env *env, int32_t max_plies, int32_t auto_reset, uint64_t *traj_state,
               uint64_t *traj_mask, int16_t *traj_action, int32_t *games_done,
               int32_t *steps_done);
/* hz_reset (all boards) fused with hz_rollout in one launch: the chance
 * streams are seeded and consumed in LDS and written to HBM once.  With
 * chance-ahead on (the default), the other blocks of the same launch run,
 * concurrently with the play, a three-stage pipeline over every board's
 * next episodes (a game's chance draws and the benchmark rule's hashes do
 * not depend on its moves): the stream seeded three calls ahead, its piles
 * drawn two and one calls ahead, with the rule hashes; a call replays the
 * prepared piles instead of seeding and drawing (identical results; a board
 * whose episode counter was moved by anything else seeds in place, a game
 * needing more piles continues on the prepared stream). */
int hz_play(hz_env *env, int32_t max_plies, int32_t auto_reset, uint64_t *traj_state,
            uint64_t *traj_mask, int16_t *traj_action, int32_t *games_done,
            int32_t *steps_done);
/* chance-ahead for hz_play: draws = piles prepared per board (0 = off,
 * capped at 24 = the default). */
int hz_env_set_seed_ahead(hz_env *env, int32_t draws);
/* hz_play's pipeline: 2 (the default; HZ_PIPELINE=1 in the environment at
 * hz_env_create makes 1 the default) = every board's game spread over
 * fifteen consecutive calls, one stage per call (seeding pass 1 in one
 * stage, pass 2 in three, each with its share of the episode's rule hashes,
 * six draw stages, five play stages), all fifteen running in each launch on
 * different episodes, so the pipeline's depth is fifteen calls: the
 * fifteenth call after a (re)start is the first to replay a fully prepared
 * episode; 1 = the chance-ahead
 * pipeline above.  Same results either way; pipeline 2 applies to calls with
 * auto_reset = 0, no trajectory outputs and max_plies >= 96 (others take
 * pipeline 1).  Returns -1 for a value other than 1 or 2. */
int hz_env_set_pipeline(hz_env *env, int32_t pipeline);
/* hz_rollout with auto_reset: on != 0 (the default, unless HZ_AR_AHEAD=0
 * at hz_env_create) lets each such call's extra blocks prepare every board's
 * episodes two and three ahead of its counter (seeded stream, pile script of
 * the first 24 draws, cursors), so that a board whose game ends starts the
 * next one from its script instead of seeding in place
 * (harmonies_engine.py:66-79 + :120-137 restated ahead of time; a game's
 * chance sequence does not depend on its moves).  Same results either way. */
int hz_env_set_auto_ahead(hz_env *env, int32_t on);
/* Both hz_play pipelines hand rows from one wave to another inside a block
 * through an LDS progress counter; a waiting wave spins at most spin_limit
 * s_sleep rounds.  A wait that gives up ORs a bit into the env's error word
 * (1: the chance-ahead seed stage's row wait, 2: k_play2's twist wave) and
 * the call's streams are then untrusted: the caller must raise.  word is a
 * device int32 the caller reads (and clears) after a sync; NULL = the
 * handle's own word.  No reference counterpart (the reference has no
 * concurrency). */
int hz_env_set_error_word(hz_env *env, int32_t *word);
/* Test knob: the spin bound of those waits (0 = the default, 2^22 rounds);
 * a bound of 1 makes waits give up almost at once. */
int hz_env_set_spin_limit(hz_env *env, int32_t limit);

/* ---- state transfer (Python facade and tests) --------------------------- */
/* export: state[6][n] and, optionally, the MT streams in CPython getstate()
 * form (mt[n][624], mt_index[n] in [0, 624]).  Finishes any partially
 * twisted generation in place (the stream's future outputs are unchanged). */
int hz_export_state(hz_env *env, uint64_t *state, uint32_t *mt, int32_t *mt_index);
/* import: the inverse; mt/mt_index may be NULL to keep the current streams. */
int hz_import_state(hz_env *env, const uint64_t *state, const uint32_t *mt, const int32_t *mt_index);

/* ---- batched MCTS (MCTS.py) ---------------------------------------------- */
/* One single-tree PUCT search per board of an hz_env, all boards advancing
 * one simulation per call sequence select -> encode_leaves -> (caller's
 * policy/value inference, e.g. PyTorch) -> expand_backup.  Semantics follow
 * get_best_action_and_pi (MCTS.py:272-441) with moves in ascending action
 * order (the reference's order is set iteration order).
 * Transpositions are keyed like the reference's hash(state) (exact_keys = 0)
 * or by the exact canonical tuple (exact_keys = 1).
 *
 * Limits (no reference counterpart: the reference's tree grows without bound;
 * this is the build's defined behaviour, restated by the C oracle's
 * or_mcts_cfg.max_nodes / max_depth and pinned by
 * tests/test_mcts_limits_gpu.py).  max_nodes bounds the nodes and, separately,
 * the edges (max_edges = max_nodes) of a board's search; 1 + sims * 69 never
 * overflows.  It must be at least 2 and below 2^24 (edge ids are packed into
 * 24 bits of the walk's hints), max_depth at least 1, else create returns
 * NULL.  max_depth bounds the edges of a simulation's path (and
 * hz_mcts_pv's max_len).
 *  - An expansion that does not fit is refused whole.  "Fits" counts what the
 *    expansion actually adds, after transposition and sibling de-duplication:
 *    nodes + new nodes <= max_nodes and edges + new edges <= max_nodes.  A
 *    refused expansion writes no node, edge or hash slot; the leaf stays
 *    unexpanded, and counts[b][3] is set to 1.
 *  - A refused leaf is still evaluated and its value backed up along the path.
 *  - A refused expansion of a place_tile_3 leaf has already replayed its
 *    children's turn-end chance draws and written the board's stream and cursor
 *    back: the draws are kept, and the same leaf draws again the next time it
 *    is selected.  The stream after a flagged search is therefore not the
 *    unbounded search's.
 *  - Each expansion is judged on its own: after a refusal a later, smaller
 *    expansion may still fit.  If the root's own expansion does not fit, every
 *    simulation tries it again and the search ends with no edges and no visits.
 *  - A walk that stands on a node with edges after max_depth edges stops there
 *    and sets counts[b][3] to 1.  That node is evaluated again and the value
 *    backed up along the max_depth edges; it is not expanded a second time.
 *  - A leaf with more than 69 legal moves (no legal position has them) is not
 *    expanded and sets counts[b][3] to 2.
 * counts[b][3] is per search: hz_mcts_begin clears it for every active board.
 * A board whose flag is 0 after a search is bit for bit the unbounded search:
 * visits, tree, counts and stream.  A flagged search is still a valid PUCT
 * search, of a truncated tree; it is no longer the reference's. */
typedef struct hz_mcts hz_mcts;
hz_mcts *hz_mcts_create(int32_t n_boards, int32_t max_nodes, int32_t max_depth, int32_t exact_keys, void *stream);
void hz_mcts_destroy(hz_mcts *mcts);
int hz_mcts_set_stream(hz_mcts *mcts, void *stream);
/* new tree per board with root = the env board's current state (MCTS.py:288);
 * active[b] == 0 (or NULL = all active) leaves board b out of this search */
int hz_mcts_begin(hz_mcts *mcts, hz_env *env, const uint8_t *active);
/* move_to_leaf (MCTS.py:63-149) for every active board */
int hz_mcts_select(hz_mcts *mcts, const uint8_t *active, float cpuct);
/* create_state_tensors of every board's selected leaf into board[n][38][5][7],
 * glob[n][42]; rows of terminal leaves / inactive boards are zero */
int hz_mcts_encode_leaves(hz_mcts *mcts, float *board, float *glob);
/* The leaves that need the network, gathered: the active boards whose
 * selected leaf is not terminal (MCTS.py:297-341 calls predict only for
 * those), in ascending board order.  count[0] (device) = k; rows[j] (may be
 * NULL, [n]) = board of row j; board[j] / glob[j] for j < k get the leaf's
 * create_state_tensors, rows >= k are not written.  No host round trip: the
 * leaf-eval kernels below take `count` as their live-row bound.  Pair with
 * hz_mcts_expand_backup_gathered. */
int hz_mcts_gather_leaves(hz_mcts *mcts, float *board, float *glob, int32_t *rows, int32_t *count);
/* hz_mcts_select followed by hz_mcts_gather_leaves (board and glob both
 * required), as one launch when the handle has at most 32 boards (config 1's
 * one-board searches, the arena): same results, two launch latencies less
 * per simulation. */
int hz_mcts_select_gather(hz_mcts *mcts, const uint8_t *active, float cpuct, float *board, float *glob,
                          int32_t *rows, int32_t *count);
/* counter (device int64, may be NULL to detach): every later
 * hz_mcts_gather_leaves adds its row count k to counter[0] on the device
 * (the number of leaf evaluations of a search without a separate kernel). */
int hz_mcts_set_eval_counter(hz_mcts *mcts, int64_t *counter);
/* Test switch (no reference counterpart): on != 0 makes every expansion's
 * sibling dedup take its serial walk instead of the LDS hash table (the path
 * the table leaves to the walk only on a hash collision), so tests can check
 * both give the same trees.  Off by default. */
int hz_mcts_set_dedup_walk(hz_mcts *mcts, int32_t on);
/* Test / A-B switch (no reference counterpart): how hz_mcts_gather_leaves
 * runs on this handle: 1 = one k_gather_encode launch, 0 = k_gather + the
 * encoder launches (same rows, slots, count and tensors), -1 = the default a
 * new handle has (the fused launch). */
int hz_mcts_set_gather_encode(hz_mcts *mcts, int32_t mode);
/* expand_leaf (MCTS.py:151-218) with policy[n][143] (probabilities, as
 * ModelManager.predict returns them, model.py:81-110), root Dirichlet mix
 * (MCTS.py:308-327) when !testing using noise[n][69] (i-th legal move), then
 * back_fill (MCTS.py:220-266) with value[n] (terminal leaves use the game
 * outcome, MCTS.py:333-341).  Children's chance draws consume the env
 * board's MT stream in child order, like the reference's apply_move calls. */
int hz_mcts_expand_backup(hz_mcts *mcts, hz_env *env, const float *policy, const float *value,
                          const double *noise, double eps, int32_t testing);
/* the same with policy[k][143] / value[k] in the row order of the last
 * hz_mcts_gather_leaves (board b reads row j where rows[j] = b) */
int hz_mcts_expand_backup_gathered(hz_mcts *mcts, hz_env *env, const float *policy, const float *value,
                                   const double *noise, double eps, int32_t testing);
/* hz_mcts_expand_backup_gathered followed by the next simulation's
 * hz_mcts_select(active, cpuct), in one launch (each board's wave walks its
 * tree right after its backup; same leaves and paths as the two calls).
 * A search then runs select once, and per simulation gather_leaves, the
 * network and this (the last simulation: hz_mcts_expand_backup_gathered).
 * Replaces the select of MCTS.py:297-305's next iteration. */
int hz_mcts_expand_backup_select(hz_mcts *mcts, hz_env *env, const float *policy, const float *value,
                                 const double *noise, double eps, int32_t testing, const uint8_t *active,
                                 float cpuct);
/* hz_mcts_expand_backup_select, then, in the same launch, the next leaf
 * batch (hz_mcts_gather_leaves' outputs): each board whose new leaf needs
 * the network takes the next row of *count_out (atomically: rows in
 * arrival order, not board order; rows[j] = board of row j, as before) and
 * encodes its leaf into board[j], glob[j].  *count_out must be 0 at launch;
 * *count_prev (the count of the batch this launch consumes) is set to 0,
 * after being added to the eval counter when add_prev != 0 (a count that no
 * gather call added).  Every result (visits, trees, streams) equals the
 * separate launches'; the evaluator must treat rows independently. */
int hz_mcts_expand_backup_select_gather(hz_mcts *mcts, hz_env *env, const float *policy, const float *value,
                                        const double *noise, double eps, int32_t testing, const uint8_t *active,
                                        float cpuct, float *board, float *glob, int32_t *rows, int32_t *count_out,
                                        int32_t *count_prev, int32_t add_prev);
/* Self-play root noise (MCTS.py:314-316, np.random.dirichlet([alpha] * L)
 * over the L = count[b] legal moves, in legal-move order) into noise[n][69]
 * (zeros past L) and the tau = 1 move-choice uniform (MCTS.py:411,
 * np.random.choice) into u[n] (may be NULL), from a counter-based generator
 * keyed by (seed, global board id = board_base + b, move): a board's draws do
 * not depend on the batch or the GPU count.  Enqueued on `stream`. */
int hz_root_noise(const int32_t *count, int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double alpha,
                  double *noise, double *u, void *stream);
/* Playout-cap coin (no reference counterpart; for a self-play that searches
 * only a random share of its moves in full, as KataGo does): coin[n] (device)
 * gets one uniform in (0, 1] per board from hz_root_noise's generator and key
 * (seed, board_base + b, move) under a salt of its own, so hz_root_noise's
 * noise and u are what they were and a board's coin depends on nothing but
 * (seed, global board id, move).  Enqueued on `stream`. */
int hz_playout_coin(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double *coin, void *stream);
/* ---- row capacity of the evaluator's outputs (no reference counterpart) -----
 * rows = the number of rows of the policy / value tensors the next expand
 * calls get (all four forms); 0 = unchecked.  Host state only: nothing is
 * launched, a launch carries the value set before it, and a launch captured in
 * a HIP graph keeps its capture's.  A board whose row (its own index, or its
 * row of the gathered batch) is at or past the cap reads neither tensor,
 * expands nothing, backs up nothing and sets bit 0 of the handle's device
 * error word.  hz_mcts_take_error waits for the handle's stream, stores the
 * word in *out (host) and clears it: a wrong bound is an error the caller
 * sees, never a read past the tensors. */
int hz_mcts_set_row_cap(hz_mcts *mcts, int32_t rows);
int hz_mcts_take_error(hz_mcts *mcts, int32_t *out);
/* ---- per-board simulation budgets (no reference counterpart) ----------------
 * budget[n] (device int32; copied into the handle in stream order) gives
 * board b at most budget[b] simulations per search; NULL turns the gate off
 * (the default).  Under the gate every select (hz_mcts_select,
 * hz_mcts_select_gather and the select inside hz_mcts_expand_backup_select /
 * _select_gather) walks board b only if it is active, has a tree and has had
 * fewer than budget[b] simulations since hz_mcts_begin, and counts the walk; a
 * spent board has no leaf: it takes no leaf row, draws nothing from its stream
 * and backs up nothing.  A refused expansion (max_nodes, max_depth) counts as
 * a simulation; a negative budget is 0; a budget above the number of sim steps
 * the caller runs is never reached.  hz_mcts_begin zeroes the counts, and
 * gives a stuck root (no legal move, game not over) budget 0 in the handle's
 * copy: its simulations would change nothing.  Call hz_mcts_set_budget before
 * the hz_mcts_begin of each search.  hz_mcts_sims_done copies the counts to
 * out[n] (device): 0 for boards left out and while the gate is off.
 * hz_mcts_set_root_noise_mask: mask[n] (device uint8, copied; NULL = every
 * board, the default): the root Dirichlet mix is applied to board b only if
 * mask[b] != 0 (and !testing and noise != NULL, as before).
 * The handle's buffers keep their addresses, so a captured simulation stays
 * valid while budgets and mask change; whether the gate and the mask are on
 * is part of what a capture holds.
 * Exactness: under the gate, a board with budget k and mask bit r after S sim
 * steps is bit for bit the search of min(k, S) simulations with testing = !r
 * (MCTS.py:288-352; the oracle's mcts_search(sims = min(k, S))): visits, node
 * and edge counts, limit flag and the board's stream. */
int hz_mcts_set_budget(hz_mcts *mcts, const int32_t *budget);
int hz_mcts_sims_done(hz_mcts *mcts, int32_t *out);
int hz_mcts_set_root_noise_mask(hz_mcts *mcts, const uint8_t *mask);
/* ---- the turn of asynchronous self-play (no reference counterpart) -----------
 * SelfPlay.play_async: a board whose search is spent records its result, plays
 * its move and begins its next search inside a sim step, while every other
 * board's tree, counters, budget and noise row stay untouched, so every sim
 * step has one live row per board.  All of it is defined under the budget gate
 * (hz_mcts_set_budget) and, where a full flag is recorded, the root-noise mask.
 * A mask here is device uint8 [n]: 1 selects the board, 0 leaves it alone;
 * hz_mcts_begin_some also knows 2.
 *
 * hz_mcts_begin_some: for mask[b] == 1 exactly what hz_mcts_begin does for an
 * active board (node 0 = the env's state, its key, its hash entry under a new
 * generation, counts[b] = {1, 0, generation + 1, 0}, sims_done[b] = 0, budget 0
 * in the handle's copy for a stuck root, the board's carry dropped); for
 * mask[b] == 0 NOTHING is written (hz_mcts_begin clears inactive boards and
 * zeroes every board's sims_done; this does not); for mask[b] == 2 the board is
 * stopped: counts[b][0] = counts[b][1] = 0, leaf -1, sims_done 0 and, under the
 * gate, budget 0, so no select walks it again.
 * hz_mcts_set_gate_some: budget_buf[b] = budget[b] and the root-noise bit of b
 * = (noise_bit[b] != 0) where mask[b] == 1, in stream order, the handle's
 * buffers keeping their addresses; either array may be NULL (not updated).
 * -1 when the gate (the mask) it would update is off.  Call it before the
 * hz_mcts_begin_some of the boards' searches.
 * hz_root_noise_at / hz_playout_coin_at: hz_root_noise and hz_playout_coin with
 * one move counter per board, move[n] (device uint64 / int64): where
 * mask[b] == 1, row b of noise, u[b] and coin[b] get the bits of the scalar
 * call with move = move[b]; every other row keeps what it holds.
 * hz_choose_actions: the move choice of get_best_action_and_pi (MCTS.py:394-423)
 * as hzamd.mcts.choose_actions computes it, from visits[n][143] by action id:
 * total and cumulative counts in int64; where explore[b] != 0 the first action
 * a with u[b] * total < cum[a], the product and both sides in fp64 (action 0 if
 * none is); else the first action with the most visits; -1 when total == 0.
 * hz_turn_choose (step 4a of a turn): board b turns iff 0 <= mc[b] < moves and
 * sims_done[b] >= the handle's budget[b].  For a turning board: its root visits
 * by action id as hz_mcts_result gives them, action[b] by hz_choose_actions'
 * rule with explore = !testing && ply[b] < turns_until_tau0, turned[b] = 1, and
 * the record row at slot k = mc[b]: rec_states[k][0..5][b] = the env's six state
 * words, rec_visits[k][b][0..142], rec_game[k][b] = game[b], and rec_full[k][b]
 * (may be NULL) = the board's root-noise bit.  Otherwise action[b] = -1,
 * turned[b] = 0 and no record is written.  -1 when the budget gate is off.
 * hz_turn_after (step 4c), after hz_step(action): for turned[b] != 0, from the
 * env's state now: rec_ended[k][b], rec_outcome[k][b] (+1 / -1 / 0 for player
 * 0 / player 1 / a draw or a game not over), rec_plies[k][b] = ply[b] + 1; then
 * game[b] += ended, ply[b] = ended ? 0 : ply[b] + 1, mc[b] = k + 1; sel[b] =
 * ended and seeds[b] = seed_base + b + (game[b] << 32) for hz_reset(sel, seeds);
 * begin[b] = 1 if mc[b] < moves, else 2 and *running -= 1; bad[b] = 1 if
 * status[b] != 0 (never cleared).  For turned[b] == 0: sel[b] = begin[b] = 0. */
int hz_mcts_begin_some(hz_mcts *mcts, hz_env *env, const uint8_t *mask);
int hz_mcts_set_gate_some(hz_mcts *mcts, const int32_t *budget, const uint8_t *noise_bit, const uint8_t *mask);
int hz_root_noise_at(const int32_t *count, int32_t n, uint64_t seed, uint64_t board_base, const uint64_t *move,
                     const uint8_t *mask, double alpha, double *noise, double *u, void *stream);
int hz_playout_coin_at(int32_t n, uint64_t seed, uint64_t board_base, const uint64_t *move, const uint8_t *mask,
                       double *coin, void *stream);
int hz_choose_actions(const int32_t *visits, int32_t n, const uint8_t *explore, const double *u, int16_t *action,
                      void *stream);
int hz_turn_choose(hz_mcts *mcts, hz_env *env, const double *u, const int32_t *ply, const int64_t *mc,
                   const int64_t *game, int64_t moves, int32_t turns_until_tau0, int32_t testing, int16_t *action,
                   uint8_t *turned, int64_t *rec_states, int32_t *rec_visits, int32_t *rec_game, uint8_t *rec_full);
int hz_turn_after(hz_env *env, const uint8_t *turned, const int32_t *status, int64_t *mc, int32_t *ply, int64_t *game,
                  int64_t moves, uint64_t seed_base, uint8_t *rec_ended, float *rec_outcome, int16_t *rec_plies,
                  uint8_t *sel, uint64_t *seeds, uint8_t *begin, uint8_t *bad, int32_t *running, void *stream);
/* ---- the Gumbel root: sequential halving, improved-policy targets ------------
 * No reference counterpart ("Policy improvement by planning with Gumbel",
 * Danihelka et al., ICLR 2022): the build's defined behaviour, off by default,
 * pinned by tests/mcts_gumbel_model.py.  Only the root's choice changes; below
 * the root the walk, the expansion and the backup are PUCT's, bit for bit.
 * Everything that decides an edge is fp64 arithmetic in the order stated here.
 *
 * hz_root_gumbel: out[n][69] (device) gets one standard Gumbel per board and
 * legal rank, g = -log(-log u) with u = (k + 1/2) 2^-52 for a 52-bit k (strictly
 * inside (0, 1): every g is finite), from hz_root_noise's generator and key
 * (seed, board_base + b, move) under a salt of its own: the noise, the
 * move-choice uniform and the coin keep their bits, and a board's draws do not
 * depend on the batch or on how board_base splits it.  Enqueued on `stream`.
 *
 * hz_mcts_set_gumbel: g[n][69] (device f64, G by legal rank) and table
 * (device int16 [max_considered + 1][n_root]) are copied in stream order into
 * buffers the handle owns; g == NULL turns the gate off (the default).  Call it
 * before the hz_mcts_begin of each search.  The buffers are allocated by the
 * first call (the table's for the largest table admitted, 70 x 32767 int16 =
 * 4.6 MB) and keep their addresses until hz_mcts_destroy, so a captured
 * simulation stays valid while G and the table change; whether the gate is on,
 * the table's shape and the two constants are held by value in a capture: a
 * capture is to be replayed only under the settings it was captured with
 * (each call rewrites the table's contents).  1 <= max_considered <= 69,
 * 1 <= n_root <= 32767, c_visit >= 0, c_scale >= 0.  The gate does not combine
 * with root noise, budgets or a carried tree (the callers refuse those).
 *   The table, built by the caller for a search of S simulations (n_root =
 * S - 1: simulation 1 expands the root and visits no edge): row m is the
 * paper's considered-visit sequence for m actions and n_root visits.  With
 * k = m and every slot's counter 0, while the row is short: max(1, int(n_root /
 * (ceil(log2 m) k))) rounds, each appending the counters of slots 0 .. k - 1
 * and then incrementing them; then k = max(2, k / 2).  Rows 0 and 1 are
 * 0, 1, 2, ...  (m 4, 8 visits): 0 0 0 0 1 1 2 2.
 *   Under the gate node 0's expansion also stores the network's fp32 value of
 * the root (v_root) and, per root edge e, score0_e = G[rank of e's move among
 * the legal moves] + log((double)P_e) (the device's log, taken this once; -inf
 * where P_e is 0).  hz_mcts_root_gumbel_scores copies score0 to out[n][69]
 * (device f64, by root edge index, 0.0 past the root's edges).
 *   Root select (level 0 of the walk, a root with ne > 0 edges; edges in
 * ascending index): t = sum N; m = min(max_considered, ne); cv =
 * table[m][min(t, n_root - 1)]; edge e is a candidate iff N_e == cv (if no edge
 * is, every edge is: a search longer than the table); score_e = max(-1e9,
 * score0_e + sigma_e); the first candidate with the largest score wins.
 *   sigma: q_e = W_e / N_e on visited edges; sp = sum (double)P_e and spq =
 * sum (double)P_e * q_e over the visited edges; v_mix = (v_root + t * (sp > 0 ?
 * spq / sp : 0)) / (t + 1); the completed q_e is q_e where visited, else v_mix;
 * mn, mx its minimum and maximum over the root's edges; sigma_e = ((c_visit +
 * max N) * c_scale) * ((q_e - mn) / max(mx - mn, 1e-8)).  Every operation is
 * one IEEE fp64 operation, none fused.  The two sums are xor butterflies over
 * 64 lanes: lane l starts with edge l's term plus edge l + 64's (0.0 for an
 * absent or unvisited edge), then v[l] = v[l] + v[l ^ off] for off = 1, 2, 4,
 * 8, 16, 32 (every lane ends with the same sum).
 *   hz_mcts_gumbel_result, after the search (device outputs): action[n] int16 =
 * the move of the first edge with the largest score among those with N_e ==
 * max N; pi[n][143] f32 = softmax over the root's edges of log P_e + sigma_e
 * (fp64, the maximum subtracted, the sum a butterfly as above; zero off the
 * root's edges; should every P_e be 0, the softmax of sigma alone); value[n]
 * f64 = v_mix.  A root without edges (stuck, terminal, left out of the search,
 * or with more than 69): action -1, a zero row, value 0.  Both reports return
 * -1 while the gate is off. */
int hz_root_gumbel(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double *out, void *stream);
int hz_mcts_set_gumbel(hz_mcts *mcts, const double *g, const int16_t *table, int32_t max_considered, int32_t n_root,
                       double c_visit, double c_scale);
int hz_mcts_root_gumbel_scores(hz_mcts *mcts, double *out);
int hz_mcts_gumbel_result(hz_mcts *mcts, int16_t *action, float *pi, double *value);
/* ---- leaf symmetries: each leaf evaluated under a random board symmetry -------
 * No reference counterpart (AlphaGo Zero's random symmetry per evaluation): the
 * build's defined behaviour, off by default, pinned by tests/mcts_leafsym_model.py.
 * The network sees each leaf in one of the board's four orientations ("board
 * symmetries" above), so its asymmetries do not always push the same way.
 *
 * hz_leaf_sym_keys: out[n] (device u64) gets one key per board, from
 * hz_root_noise's generator and board key (seed, board_base + b, move) under a
 * salt of its own: key = mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908) ^
 * (board_base + b)) ^ move), out[b] = mix64(key ^ 0xC2B2AE3D27D4EB4F), mix64 the
 * splitmix64 finalizer.  The noise, the move-choice uniform, the coin and the
 * Gumbels keep their bits, and a board's key does not depend on the batch or on
 * how board_base splits it.  Enqueued on `stream`.
 *
 * hz_mcts_set_leaf_symmetry: key[n] (device u64) is copied in stream order into
 * a buffer the handle owns; key == NULL turns the gate off (the default).  Call
 * it before the hz_mcts_begin of a search.  The buffers are allocated by the
 * first call and keep their addresses until hz_mcts_destroy, so a captured
 * simulation stays valid while the keys change; whether the gate is on is held
 * by value in a capture, which is to be replayed only under the gate it was
 * captured with.
 *   The rule.  The symmetry of board b's leaf is a pure function of the key and
 * the leaf's node id in the board's pool:
 *     g = mix64(key[b] ^ (0x9FB21C651E98DF25 * (node + 1))) >> 62
 * (64-bit wrapping arithmetic).  A node is evaluated at most once per search,
 * and a refused expansion repeats with the same g; the rule needs no simulation
 * counter, so it is the same in every search form and under graph replay; the
 * side that encodes a leaf and the side that expands it compute g on their own.
 *   Under the gate the row encoded for a leaf, by every call that encodes
 * leaves (hz_mcts_encode_leaves, hz_mcts_gather_leaves in both forms,
 * hz_mcts_select_gather, hz_mcts_expand_backup_select_gather), is the encoding
 * of the leaf's state under g, and the expansion reads the prior of action a at
 * policy[row][a under g] (every g is its own inverse).  The value is read as it
 * is.  Nothing else changes: the walk, the children (built from the leaf as
 * stored), keys, transpositions, chance draws, root noise by legal rank, backup
 * and limits are what they are without the gate.
 *   The gate does not combine with the Gumbel root: with both on, the calls
 * that select-and-gather or expand return -1 and enqueue nothing.
 *
 * hz_mcts_leaf_symmetry: out[n] (device u8) gets the g of each board's current
 * leaf; 0 for a board without a leaf to evaluate (inactive, terminal leaf,
 * budget spent) and for every board while the gate is off.  A report for
 * callers and tests, enqueued on the handle's stream. */
int hz_leaf_sym_keys(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, uint64_t *out, void *stream);
int hz_mcts_set_leaf_symmetry(hz_mcts *mcts, const uint64_t *key);
int hz_mcts_leaf_symmetry(hz_mcts *mcts, uint8_t *out);
/* ---- forced playouts at the root, policy target pruning ------------------------
 * No reference counterpart ("Accelerating Self-Play Learning in Go", Wu, 2019:
 * KataGo's companions of playout-cap randomization): the build's defined
 * behaviour, off by default, pinned by tests/mcts_forced_model.py.  A root child
 * that has been visited at all is owed sqrt(k P sum N) visits and is chosen ahead
 * of PUCT until it has them, so a move the Dirichlet noise pushed up is confirmed
 * or refuted; after the search the visits that were only forced are taken back.
 * Both rules are root-only and use IEEE fp64 multiply, divide, add and sqrt, one
 * operation at a time, none fused, on numbers the walk already holds.
 *
 * hz_mcts_set_forced: k > 0 turns the gate on; mask[n] (device uint8) is copied in
 * stream order into a buffer the handle owns (allocated by the first call, its
 * address fixed until hz_mcts_destroy); mask == NULL: every board.  k == 0 turns
 * the gate off (the default); a negative or NaN k returns -1.  Call it before the
 * hz_mcts_begin of a search.  k, whether the gate is on and whether the mask is
 * NULL are held by value in a captured simulation (a capture made with a mask
 * reads the handle's buffer, one made without reads none), which is to be
 * replayed only under the settings it was captured with; the mask's contents may
 * change between replays.  The gate does not combine with the Gumbel root (with both on,
 * every call that selects or expands returns -1 and enqueues nothing) or with a
 * carried tree (hz_mcts_begin_carried returns -1); it combines with budgets, the
 * root-noise mask, the row cap and leaf symmetries.
 *   Forced select: level 0 of the walk, a board whose bit is set and whose root
 * has 1 <= ne <= 69 edges; t = sum N over the root's edges.  Edge e is forced iff
 * N_e > 0 and (double)(N_e * N_e) < (k * (double)P_e) * (double)t: an exact integer
 * product on the left, two fp64 multiplications in that order on the right, P_e
 * the stored prior (after the root mix).  If any edge is forced, the first forced
 * edge in ascending edge index wins; otherwise the choice is PUCT's, unchanged.
 * Every other level, the expansion, the draws, the backup, the budgets and the
 * limits are what they are without the gate, and a board whose bit is clear
 * searches exactly as it does without it.
 *   hz_mcts_pruned_visits (enqueued on the handle's stream; -1 while the gate is
 * off): visits[n][143] (device int32) by action id.  For a board whose bit is set,
 * whose root has edges and t > 0: s = sqrt(max(1, t)); U_e(x) = ((double)(cpuct
 * *f32 P_e) * s) / (double)(1 + x) and q_e = N_e ? W_e / N_e : 0, the select's own
 * arithmetic; e* = the first edge with the largest N, bound = q_e* + U_e*(N_e*).
 * Every other edge with N_e > 0: nf = (int)floor(sqrt((k * (double)P_e) *
 * (double)t)); r = the largest value in 0 .. min(nf, N_e) such that q_e +
 * U_e(N_e - j) < bound for every j = 1 .. r (the first j that fails ends it; q_e
 * stays fixed); N'_e = N_e - r, and 0 if r > 0 and N'_e <= 1.  e* and unvisited
 * edges keep their counts.  A board whose bit is clear gets hz_mcts_result's row;
 * a board without a tree zeros.
 *   hz_mcts_forced_counts (a report for callers and tools; -1 while the gate is
 * off): out[n][2] (device int32) = per board, the root selections this gate saw
 * since the last hz_mcts_set_forced (a board whose bit is set, a root with edges)
 * and those of them the forced rule decided.  The counters are instrumentation
 * that stays in the forced kernels: lane 0 of the board's wave adds to them at
 * every root selection under the gate (kernels of a handle with the gate off hold
 * no such code).  A separate instantiation without them is a possible follow-up. */
int hz_mcts_set_forced(hz_mcts *mcts, const uint8_t *mask, double k);
int hz_mcts_pruned_visits(hz_mcts *mcts, float cpuct, int32_t *visits);
int hz_mcts_forced_counts(hz_mcts *mcts, int32_t *out);
/* ---- tree reuse: the searched subtree carried into the next search ----------
 * No reference counterpart (MCTS.py:288 builds a fresh Node per call): this is
 * the build's defined behaviour, off unless the caller asks for it, pinned by
 * tests/test_mcts_carry_gpu.py against the host model tests/mcts_carry_model.py.
 *
 * hz_mcts_advance is called after hz_step has applied action[n] (device int16)
 * to the env.  Board b is CARRIED iff all of these hold:
 *  - active[b] != 0 (NULL: every board), its last search left a tree, and
 *    action[b] >= 0;
 *  - the root has an edge for action[b];
 *  - that edge's child c is not terminal;
 *  - node_state[c] equals the env's current state of b in all six words.  This
 *    is the rule, not an optimisation: a place_tile_3 child refilled its pile
 *    from draws taken when it was expanded, hz_step draws again from where the
 *    stream then stands, so a turn end carries only when the draws agree; pile
 *    choice and the first two placements are deterministic and carry;
 *  - kept nodes + headroom <= max_nodes and kept edges + headroom <= max_edges
 *    (headroom >= 0, else -1; 69 * sims cannot overflow in the next search).
 * Otherwise it is DROPPED: carry flag 0, counts[b][0..1] = 0, info[b] = {0,0,0}.
 * For a carried board the tree becomes the sub-DAG reachable from c.  The result
 * is defined by this rule, not by a traversal order:
 *  - Nodes: c becomes node 0; the other kept nodes take ids 1.. in ascending old
 *    id.  State and canonical key move with their node.
 *  - Edges: the edge blocks of the kept expanded nodes keep their relative pool
 *    order and are packed from 0.  A node's first edge and every edge's child
 *    are renumbered (a node without edges has first edge 0); action, N, W, P and
 *    mover move unchanged, bit for bit.
 *  - The generation counts[b][2] is incremented and every kept node entered into
 *    the hash table again.  Dropped nodes are gone: a later expansion that would
 *    have transposed onto one makes a new node.
 *  - The walk's hints are rebuilt from the moved nodes.
 *  - counts[b] = {kept nodes, kept edges, generation, 0}; info[b] (device int32
 *    [n][3]) = {kept nodes, kept edges, sum of N over the new root's edges}; the
 *    board's carry flag is set in the handle.
 * The move is done in place with two int32 [n][max_nodes] scratch arrays the
 * first call allocates (no second node pool).  One launch, no synchronisation.
 *
 * hz_mcts_begin_carried starts the next search in place of hz_mcts_begin:
 *  - a board whose carry flag is set and whose node 0 still equals the env's
 *    state (checked again: a reset or import in between drops the carry) keeps
 *    its tree; its limit flag and simulation count are cleared, and the stuck-
 *    root budget rule of hz_mcts_begin applies unchanged;
 *  - if that root is expanded and the board is noisy (!testing, noise != NULL,
 *    no mask or mask[b]), the root priors are mixed once with the expansion's
 *    arithmetic: P = f32(f64(f32(1 - eps) * P) + eps * noise[b*69 + i]), i the
 *    rank of the edge's action among the root's legal moves (not the edge index:
 *    a skipped self-loop child shifts it).  A carried root without edges is
 *    expanded by the first simulation and mixed there, as any root;
 *  - every other active board gets exactly what hz_mcts_begin does;
 *  - the flag is consumed either way: a second hz_mcts_begin_carried without an
 *    hz_mcts_advance starts fresh.
 * hz_mcts_begin always starts fresh and clears the flags.  The simulations of a
 * carried search are the ones of any search: nothing in select, expand or backup
 * knows about the carry. */
int hz_mcts_advance(hz_mcts *mcts, hz_env *env, const int16_t *action, const uint8_t *active, int32_t headroom,
                    int32_t *info);
int hz_mcts_begin_carried(hz_mcts *mcts, hz_env *env, const uint8_t *active, const double *noise, double eps,
                          int32_t testing);
/* root visit counts by action id: visits[n][143] (MCTS.py:355-376) */
int hz_mcts_result(hz_mcts *mcts, int32_t *visits);
/* per-board [nodes, edges, search generation, limit flag] -> counts[n][4].
 * The limit flag (hz_mcts_create, "Limits"): 0 = this search is the unbounded
 * search; 1 = an expansion did not fit max_nodes or a walk reached max_depth;
 * 2 = a leaf had more than 69 legal moves.  Cleared by hz_mcts_begin for the
 * boards it starts (a board left out keeps counts 0, 0 and its last flag). */
int hz_mcts_stats(hz_mcts *mcts, int32_t *counts);
/* ---- search report: three read-only views of the trees ---------------------
 * None writes the tree, the env or the streams; each is enqueued on the
 * handle's stream without synchronising, can be captured in a HIP graph, and
 * is valid at any point between the calls of a search once hz_mcts_begin has
 * run (before it every board reads as left out).  Node and edge ids read from
 * the tree are checked against the board's counts before they are used. */
/* MCTS.get_root_edges (MCTS.py:268-269) by action id, what Edge.stats holds
 * (MCTS.py:34-39): n[n][143] (equals hz_mcts_result), w[n][143] the stored
 * fp64 W, q[n][143] = W / N as back_fill's last update left it (MCTS.py:254,
 * one fp64 division; 0.0 while N == 0), p[n][143] the stored fp32 prior (the
 * root's after the Dirichlet mix, MCTS.py:323), child[n][143] (may be NULL)
 * the edge's child node id, value[n] (may be NULL) = sum W / sum N over the
 * root's edges, both sums taken in ascending edge order in fp64 (0.0 when
 * sum N is 0), from the root mover's side.  An action without a root edge
 * (illegal, a skipped self-loop child of MCTS.py:189-194, a board left out of
 * the search, a stuck, terminal or unexpanded root) gets 0, 0.0, 0.0, 0.0 and
 * child -1. */
int hz_mcts_root_edges(hz_mcts *mcts, int32_t *n, double *w, double *q, float *p, int32_t *child, double *value);
/* The principal variation: from the root, at every node the edge with the
 * most visits, the first in edge (= ascending action) order among equals, as
 * the greedy move choice of MCTS.py:418-423 picks at the root; the line ends
 * at a node without edges, at an edge with N == 0, at a link outside the
 * board's tree, or after max_len moves (1 <= max_len <= the handle's
 * max_depth, else -1).  action[n][max_len], visits[n][max_len] (the edge's
 * N), q[n][max_len] (its W / N), player[n][max_len] (its mover,
 * Edge.current_player MCTS.py:29-31), len[n]; entries at and past len[b] are
 * -1, 0, 0.0 and 0. */
int hz_mcts_pv(hz_mcts *mcts, int32_t max_len, int16_t *action, int32_t *visits, double *q, uint8_t *player,
               int32_t *len);
/* Board b's whole node and edge slices (Node MCTS.py:8-20, Edge :23-39),
 * copied in stream order into device buffers of max_nodes entries each (any
 * may be NULL): node_state[max_nodes][6], node_e0 / node_ne (a node's first
 * edge and edge count; ne = -1 marks a terminal node, 0 an unexpanded one);
 * per edge its action, child node, N, W, P and mover.  Entries past the
 * board's node / edge counts (hz_mcts_stats) are stale: the caller trims. */
int hz_mcts_export_tree(hz_mcts *mcts, int32_t b, uint64_t *node_state, int32_t *node_e0, int32_t *node_ne,
                        int16_t *edge_action, int32_t *edge_child, int32_t *edge_n, double *edge_w, float *edge_p,
                        uint8_t *edge_player);
/* out[0] (device int64) += the sum of every edge's visit count over every
 * board's current tree, i.e. the edge levels its simulations walked (each
 * back_fill, MCTS.py:220-266, visits every edge of its path once): the
 * path-walk term of the tree kernels' algorithmic bytes (bench.py). */
int hz_mcts_path_edges(hz_mcts *mcts, int64_t *out);
/* Test entry point: the transposition keys the search builds incrementally
 * (canon_key_child, from the parent's key) against keys built from the child's
 * state (canon_key).  states: device [6][n] state words (hz_export_state's
 * layout).  For every legal action a of every unfinished state, the child is
 * made by the step rule (a turn-ending child draws its piles from a script
 * fixed by (b, a)) and both keys are built in both key forms (exact and
 * Python-hash).  Adds to the device counters out[0..2]: pairs checked, pairs
 * with a key mismatch or a failed step, pairs whose step failed.  One launch
 * enqueued on `stream` (hipStream_t, NULL = null stream); no synchronisation. */
int hz_key_check(const uint64_t *states, int32_t n, int64_t *out, void *stream);
/* host pointers to the device arrays leaf[n] / leaf_gidx[n] (debugging) */
int hz_mcts_leaf_ptrs(hz_mcts *mcts, int32_t **leaf, int32_t **leaf_gidx);

/* ---- leaf-eval kernels (hzamd/infer.py) ---------------------------------- */
/* `live` (device pointer, may be NULL) bounds the rows computed: rows
 * >= min(batch, *live) are neither read nor written (gathered leaf batches
 * whose size is known only on the device). */
/* x[rows][ch] = relu((x + bias[c]) + res) in place (res may be NULL): the
 * eval-mode BatchNorm (folded into the conv) -> [+ skip] -> ReLU tail of
 * model.py:376-393 (ResidualBlock.forward) and model.py:325-330 (stem) over an
 * NHWC activation.  ch % 4 == 0, pointers 16-byte aligned. */
int hz_bias_act(float *x, const float *bias, const float *res, int64_t rows, int32_t ch, void *stream);

/* out = relu((conv3x3(x, w) + bias[co]) + res) for the residual tower's
 * 128 -> 128 channel convs (model.py:362-371, kernel 3, padding 1) on the
 * 5x7 board: x, res, out NHWC [batch][5][7][128] (res may be NULL; out must
 * not alias x or res), wpack = w[co][ci][kh][kw] repacked as
 * [kh*3+kw][ci/16][co][ci%16] (hzamd/infer.py:pack_conv3x3).  f32 MFMA, exact
 * fp32 products and sums (summation order differs from MIOpen's). */
int hz_conv3x3_bias_act(const float *x, const float *wpack, const float *bias, const float *res, float *out,
                        int32_t batch, const int32_t *live, void *stream);

/* hz_conv3x3_bias_act on the bf16 MFMA (v_mfma_f32_16x16x32_bf16) with
 * fp32-exact products: x and w are split exactly into three bf16 pieces each
 * and the six piece products of order <= 2 are accumulated in fp32 (the
 * dropped ones are below one fp32 rounding).  wpack6 = bf16 planes
 * [kh*3+kw][ci/32][plane h,m,l][co][ci%32] (hzamd/infer.py:pack_conv3x3_x6). */
int hz_conv3x3_x6_bias_act(const float *x, const void *wpack6, const float *bias, const float *res, float *out,
                           int32_t batch, const int32_t *live, void *stream);

/* hz_conv3x3_x6_bias_act keeping only the piece products of order
 * <= {1:0, 3:1, 6:2}; products = 6 is hz_conv3x3_x6_bias_act itself.
 * products = 3 keeps h*h, h*m, m*h (|error| <= 3 * 2^-18 |x||w| per product,
 * half the MFMAs), products = 1 keeps h*h (plain bf16 operands, a sixth of
 * them).  wpack6 is the same pack_conv3x3_x6 layout (the unused planes are
 * not read); the kept products are accumulated in hz_conv3x3_x6_bias_act's
 * order, always by its generic one- and eight-state kernels.  Any other
 * `products` returns -1 with nothing enqueued. */
int hz_conv3x3_xn_bias_act(const float *x, const void *wpack6, const float *bias, const float *res,
                           float *out, int32_t batch, const int32_t *live, int32_t products, void *stream);

/* One residual block of the tower (model.py:376-393, ResidualBlock.forward
 * with BN folded): out = relu(conv2(relu(conv1(x) + b1)) + b2 + x), w1/w2
 * packed as for hz_conv3x3_x6_bias_act; x, out NHWC [batch][5][7][128] (out
 * must not alias x); tmp = scratch of batch*35*128 floats.  Bit-identical to
 * hz_conv3x3_x6_bias_act(x, w1, b1, NULL, tmp) followed by
 * hz_conv3x3_x6_bias_act(tmp, w2, b2, x, out); in its one-launch form
 * (hz_resblock_x6_fused(batch) == 1) the intermediate activation stays on
 * the CU (tmp holds half of it, briefly: a [2][288][32]-float slice per
 * 8-state group, which the one-launch form is taken only to fit in the
 * batch*35*128 floats above, i.e. never below 5 rows). */
int hz_resblock_x6_bias_act(const float *x, const void *w1, const float *b1, const void *w2, const float *b2,
                            float *out, float *tmp, int32_t batch, const int32_t *live, void *stream);
int32_t hz_resblock_x6_fused(int32_t batch);
/* on = 1 (the default, unless HZ_X6_BLOCK=0): hz_resblock_x6_bias_act takes
 * the one-launch form where it applies; 0: the two layered convs (A/B
 * measurements); results are bit-identical. */
int hz_resblock_x6_set_fused(int32_t on);
/* The one-launch form's row placement: 1 (the default, unless
 * HZ_BLK_TABLE=0) the LDS-bank-conflict-free row table the layered conv
 * uses, 0 round 3's (A/B measurements; results are bit-identical). */
int hz_resblock_x6_set_table(int32_t cf);
/* The residual tower (model.py:332-334: nblk <= 16 ResidualBlock.forward,
 * :376-393) in ONE launch where
 * hz_resblock_x6_fused(batch) holds: each workgroup carries its 8 states
 * through every block, block k's output written over block k-1's in out
 * (block 0 reads x, which is only read).  w1/b1/w2/b2 are HOST arrays of
 * nblk device pointers (each block's packed conv weights and folded
 * biases, as hz_resblock_x6_bias_act takes them); tmp as there.  The same
 * bits as nblk hz_resblock_x6_bias_act calls.  Returns -2 (nothing
 * enqueued) for a batch the per-block path serves. */
int hz_tower_x6_blocks(const float *x, const void *const *w1, const float *const *b1, const void *const *w2,
                       const float *const *b2, int32_t nblk, float *out, float *tmp, int32_t batch,
                       const int32_t *live, void *stream);
/* A/B knob (no reference counterpart): hz_tower_x6_blocks' first-round
 * workgroups on every other CU of each XCD start `units` x 8,128 cycles late
 * (default 4, HZ_TOWER_STAGGER overrides; 0: none), so the blocks' epilogue
 * bursts of all CUs stop coinciding.  Results are the same bits either way. */
int hz_tower_x6_set_stagger(int32_t units);

/* out = relu(conv3x3(board, w) + bias[co]) for the stem (model.py:328-330,
 * 38 -> 128 channels, padding 1): board NCHW [batch][38][5][7] as the
 * encoder writes it, out NHWC [batch][5][7][128], wpack = w with the input
 * channels zero-padded to 48, packed as for hz_conv3x3_bias_act. */
int hz_stem3x3_bias_act(const float *board, const float *wpack, const float *bias, float *out, int32_t batch,
                        const int32_t *live, void *stream);
/* the stem on the bf16 MFMA with fp32-exact products (as hz_conv3x3_x6_bias_act);
 * wpack6 = w with the input channels zero-padded to 64, packed as there
 * (hzamd/infer.py:pack_stem_x6). */
int hz_stem3x3_x6_bias_act(const float *board, const void *wpack6, const float *bias, float *out, int32_t batch,
                           const int32_t *live, void *stream);
/* The whole residual tower (model.py:332-333 over ResidualBlock.forward,
 * model.py:376-393, BN folded) in one launch for small batches: nconv
 * (even) convs, conv 2i without and 2i+1 with the skip of block i's input;
 * x0 = the stem's output, out = the tower's, both NHWC [batch][5][7][128]
 * (distinct buffers).  wpack6 = the nconv convs' pack_conv3x3_x6 layouts
 * back to back, bias [nconv][128].  One workgroup per state, activations
 * resident in LDS; bit-identical to nconv hz_conv3x3_x6_bias_act calls. */
int hz_tower_x6_resident(const float *x0, const void *wpack6, const float *bias, float *out, int32_t nconv,
                         int32_t batch, const int32_t *live, void *stream);
/* hz_tower_x6_resident with hz_conv3x3_xn_bias_act's `products` (1, 3 or 6;
 * 6 is hz_tower_x6_resident itself): activations between the convs are kept
 * as the planes the mode reads.  Bit-identical to nconv
 * hz_conv3x3_xn_bias_act calls with the same `products`. */
int hz_tower_xn_resident(const float *x0, const void *wpack6, const float *bias, float *out, int32_t nconv,
                         int32_t batch, const int32_t *live, int32_t products, void *stream);
/* hz_tower_x6_resident for batch <= 32 with 24 (batch <= 10) or 8
 * workgroups per state (16 output channels each) exchanging each conv's
 * output through HBM in-launch: xch = scratch of 2 * batch * 35 * 128
 * floats, sync = 33 * 32 words, zero-initialised ONCE by the caller and left
 * zeroed by every launch (calls sharing one sync block must be ordered on
 * one stream); sync[32 * 32] != 0 means a workgroup gave up waiting (1 s)
 * since the block was zeroed, and that state's output is NaN.  Bit-identical
 * to hz_tower_x6_resident. */
int hz_tower_x6_split(const float *x0, const void *wpack6, const float *bias, float *out, float *xch, uint32_t *sync,
                      int32_t nconv, int32_t batch, const int32_t *live, void *stream);

/* Every workgroup of an hz_tower_x6_split launch must be resident at once
 * (its hand-offs wait on all of them).  hz_tower_x6_split returns
 * HZ_E_NOT_RESIDENT (-2), enqueuing nothing, when the launch's grid
 * (24 workgroups per state up to 10 states, else 8) exceeds what the current
 * device holds at once (CU count x the kernel's occupancy per CU, from the
 * occupancy API) or the limit set here; callers then take
 * hz_tower_x6_resident.  max_batch: the largest batch up to which it accepts
 * every batch on the current device (0: none).  set_limit: cap the workgroups (0 = no cap
 * beyond the device's), e.g. when other work shares the GPU. */
int32_t hz_tower_x6_split_max_batch(void);
int hz_tower_x6_split_set_limit(int32_t groups);

/* The heads of model.py:336-351 up to their linear layers, BN folded:
 * pcat[b] = relu(hw[0..1] . x[b][cell] + hb[0..1]) in NCHW flatten order (70)
 * || glob[b] (42); vcat[b] = relu(hw[2] . x[b][cell] + hb[2]) (35) || glob[b].
 * x NHWC [batch][5][7][128] (16-byte aligned), hw [3][128], hb [3]. */
int hz_heads(const float *x, const float *hw, const float *hb, const float *glob, float *pcat, float *vcat,
             int32_t batch, const int32_t *live, void *stream);
/* The whole head for the default shapes (2 + 1 head filters, 143 actions,
 * 256 hidden units, 42 globals): the 1x1 convs as hz_heads, then
 * logits = pcat . wpT + bp (model.py:341-344; wpT = policy_fc.weight^T
 * [112][143]), value = tanh(w2 . relu(vcat . w1T + b1) + b2) (model.py:352-355;
 * w1T [77][256], w2 [256], b2 [1]) and ModelManager.predict's softmax
 * (model.py:100-104).  logits [batch][143] and probs [batch][143] are
 * optional (NULL: not written); value [batch]. */
int hz_heads_fc(const float *x, const float *glob, const float *hw, const float *hb, const float *wpT,
                const float *bp, const float *w1T, const float *b1, const float *w2, const float *b2, float *logits,
                float *probs, float *value, int32_t batch, const int32_t *live, void *stream);

/* ---- other filter counts and head shapes (csrc/hz_net_wide.hip) ---------- */
/* hz_conv3x3_xn_bias_act for the tower convs of a network with another
 * cnn_filters (model.py:362-371 with ch = cin = cout; model.py:376-393 for
 * the skip): cin, cout multiples of 32 in [32, 256], x NHWC
 * [batch][5][7][cin], res, out NHWC [batch][5][7][cout] (res may be NULL; out
 * must not alias x or res), wpack6 = bf16 planes
 * [kh*3+kw][cin/32][plane h,m,l][cout][cin%32] (hzamd/infer.py:pack_conv3x3_x6),
 * products as in hz_conv3x3_xn_bias_act.  Per output element the products are
 * accumulated in hz_conv3x3_x6_bias_act's order (chunks of 32 input channels
 * ascending, taps 0..8, plane pairs pa outer, pb inner), so at cin = cout =
 * 128 the result is that kernel's (products 6) or hz_conv3x3_xn_bias_act's
 * (3, 1) bit for bit.  Two workgroup forms with identical bits: one state per
 * workgroup, or eight (280 rows share each weight fragment).
 * spg: 0 = chosen by batch (one state per workgroup up to a row count that
 * falls with cin * cout: 7,550 at 32 x 32, 2,887 at 64 x 64, 422 at 256 x 256;
 * HZ_X6G_SMALL_MAX overrides it for every width), 1 or 8 = forced (tests, A/B).  -1, nothing enqueued: cin/cout not a
 * multiple of 32 in [32, 256], products not in {1,3,6}, spg not in {0,1,8}, batch < 0. */
int hz_conv3x3_x6g_bias_act(const float *x, const void *wpack6, const float *bias, const float *res, float *out,
                            int32_t cin, int32_t cout, int32_t batch, const int32_t *live, int32_t products,
                            int32_t spg, void *stream);
/* The stem (model.py:328-330, 38 -> cout channels, padding 1) for those
 * networks, all six piece products: board NCHW [batch][38][5][7] as the
 * encoder writes it, out NHWC [batch][5][7][cout]; wpack6 = w with the input
 * channels zero-padded to 64, packed as above (hzamd/infer.py:pack_stem_x6g).
 * Channel 37 (phase / 3) is split like any other value; not the 128-wide
 * stem's bits (that one packs its second chunk by taps).  spg and the
 * refusals as above. */
int hz_stem3x3_x6g_bias_act(const float *board, const void *wpack6, const float *bias, float *out, int32_t cout,
                            int32_t batch, const int32_t *live, int32_t spg, void *stream);
/* hz_heads_fc for other shapes (model.py:336-355, BN folded; predict's
 * softmax, model.py:100-104): x NHWC [batch][5][7][ch], hw [pf + vf][ch]
 * (policy filters first), hb [pf + vf], wpT = policy_fc.weight^T
 * [pf*35 + 42][143], w1T = value_fc1.weight^T [vf*35 + 42][hidden], w2
 * [hidden], b2 [1]; logits and probs optional (NULL: not written), value
 * [batch].  fp32 FMAs, each sum in one order whatever the batch or live (not
 * hz_heads_fc's bits).  -1, nothing enqueued: ch as cin above, pf or vf
 * outside 1..4, hidden outside 1..1024, batch < 0. */
int hz_heads_fc_g(const float *x, const float *glob, const float *hw, const float *hb, const float *wpT,
                  const float *bp, const float *w1T, const float *b1, const float *w2, const float *b2, float *logits,
                  float *probs, float *value, int32_t ch, int32_t pf, int32_t vf, int32_t hidden, int32_t batch,
                  const int32_t *live, void *stream);

/* ---- build info ---------------------------------------------------------- */
const char *hz_version(void);

#ifdef __cplusplus
}
#endif
#endif
