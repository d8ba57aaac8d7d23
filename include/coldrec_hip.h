/*
 * coldrec_hip.h -- C ABI of libcoldrec_hip.so (MI355X / gfx950).
 *
 * The upstream project (YuanchenBei/ColdRec) is pure Python and has NO FFI of its own; the
 * hot path is a handful of PyTorch calls.  Each entry point below names the reference call
 * site it replaces (file:line relative to the upstream repository); INTEGRATION.md shows the
 * ctypes binding a ColdRec maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - nothing is allocated or freed here: the caller owns every buffer (PyTorch's caching
 *     allocator in our host layer); scratch is passed in after a *_workspace_bytes() query;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default);
 *   - return 0 on success, <0 on error; crh_last_error() gives the thread-local message;
 *   - item / user ids are int32 (catalogues up to 2^31-2 rows); row offsets are int64.
 *   - top-k lists are ordered by the CANONICAL key (score descending, global item index
 *     ascending); lists with fewer than k candidates are padded with (-inf, CRH_PAD_IDX).
 */
#ifndef COLDREC_HIP_H
#define COLDREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRH_OK 0
#define CRH_ERR_ARG (-1)     /* bad argument (NULL, unsupported d / k, misaligned pointer) */
#define CRH_ERR_HIP (-2)     /* a HIP runtime call failed */
#define CRH_ERR_WS (-3)      /* workspace too small */
#define CRH_PAD_IDX 0x7fffffff
#define CRH_MASKED_SCORE (-1.0e9f) /* -10e8, model/BaseRecommender.py:177,180 */
#define CRH_MAX_K 128

const char* crh_last_error(void);
int crh_version(void);
/* 1 when the embedding width is handled by the MFMA kernel without padding (8,16,32,64,128,256) */
int crh_score_topk_supports_dim(int d);

/*
 * Fused full-catalogue scoring + masking + top-k for one block of users against one item shard.
 * Replaces, per user block of BaseColdStartTrainer._evaluate (model/BaseRecommender.py:172-183):
 *     batch_predict:  user_emb[users] @ item_emb.T            model/MF.py:58-63 (+21 copies)
 *     S[j, rated_j] = -10e8 ; S[:, candidate_mask] = -10e8    model/BaseRecommender.py:175-180
 *     torch.topk(S, max_N, dim=1, largest=True, sorted=True)  model/BaseRecommender.py:182
 * without materialising S.  score(u,i) is the fp32 k-ascending fma chain (exact fp32 MFMA).
 *
 *   user_emb   (n_user_rows, d) fp32 row-major, 16-byte aligned
 *   users      (n_users) int32 rows of user_emb for the block, or NULL for rows 0..n_users-1
 *   item_emb   (n_items, d) fp32: rows [item_base, item_base+n_items) of the item table
 *   rated_rowptr (n_users+1) int64 / rated_col int32: per block slot, the GLOBAL ids of the
 *              user's training items, ascending within a row; both NULL = nothing rated
 *   cand_bitmap  bit (gi & 31) of word gi>>5 set => global item gi is masked; NULL = none
 *   k          1..CRH_MAX_K;  out_score/out_idx (n_users, k), idx are GLOBAL item ids
 *   workspace  crh_score_topk_workspace_bytes(...) bytes: partial lists of the item-range splits plus a
 *              copy of the shard in MFMA-fragment order (n_items*d*4 bytes, written once per call by a
 *              streaming kernel; removes every cross-lane shuffle from the scoring loop).  With only
 *              crh_score_topk_min_workspace_bytes(...) the row-major kernel runs: identical results.
 *              Calls of up to 5e9 (user, item) pairs and 262144 items -- and any user count up to 32768 items: the
 *              trainers' per-epoch validation -- take another route when the
 *              full workspace is given and n_splits is 0: the MFMA kernel writes the score block (n_users x
 *              ceil32(n_items) fp32, at most 8 GiB at a time) into the workspace and the wave-per-user ranking of
 *              crh_mask_topk_f32 selects from it -- same scores, masks and order, ~10-30x lower latency at these
 *              sizes, where the fused selection is bound by its per-candidate slow path.
 */
size_t crh_score_topk_workspace_bytes(int64_t n_users, int64_t n_items, int d, int k);
size_t crh_score_topk_min_workspace_bytes(int64_t n_users, int k);

/* Which kernels a crh_score_topk_{f32,f16}[_ex] call of this shape takes, answered by the dispatcher's own code (the same
 * predicates and environment switches, no GPU work): the library reports its route, callers do not re-derive it.
 *   elem_bytes 4 (fp32 tables) | 2 (fp16);  workspace_bytes as it will be passed (0 = no workspace);  has_bitmap: a
 *   candidate bitmap will be passed;  n_splits as in the _ex calls (0 = library's choice).
 * Returns the route of the stage that walks the catalogue -- CRH_ROUTE_DENSE (score block + crh_mask_topk_f32),
 * CRH_ROUTE_FUSED_WAVE (one wave per user group), CRH_ROUTE_FUSED_WG (8-wave workgroups, register-staged LDS ring),
 * CRH_ROUTE_FUSED_DMA (4-wave workgroups fed by LDS-DMA) -- OR-ed with CRH_ROUTE_SEEDED when a catalogue prefix is ranked
 * first and seeds the lists, and with CRH_ROUTE_DMA_FLAGS when the DMA kernel runs in its flag form (ring slots guarded by
 * LDS counters instead of a barrier per tile: fp32 d=128 below 6 M items); < 0 on bad arguments.  prefix_items / picked_splits (either may be NULL) receive the prefix
 * length (0: not seeded) and the item-range cut count of the main stage.
 * There is no counterpart in the reference (model/BaseRecommender.py:172-183 is one matmul + topk whatever the shape). */
#define CRH_ROUTE_DENSE 1
#define CRH_ROUTE_FUSED_WAVE 2
#define CRH_ROUTE_FUSED_WG 3
#define CRH_ROUTE_FUSED_DMA 4
#define CRH_ROUTE_SEEDED 16
#define CRH_ROUTE_DMA_FLAGS 32
int crh_score_topk_route(int elem_bytes, int64_t n_users, int64_t n_items, int d, int k, size_t workspace_bytes,
                         int has_bitmap, int n_splits, int64_t* prefix_items, int* picked_splits);
/* kernel-name prefix of a route's scoring kernel as rocprofv3 prints it ("score_topk_dma_kernel", ...) */
const char* crh_score_topk_route_kernel(int route);
/* The SCREENED route of fp32 d=128 calls with k <= 20 (the headline shape): the catalogue is ranked in fp16 by the LDS-DMA kernel
 * into 28 candidates per user, the candidates are rescored with the canonical fmaf chain, and a per-user error bound proves that
 * no other item can enter the top-k; users without that proof are ranked by an exact fallback.  Results are identical to the
 * exact route's.  CRH_SCORE_SCREEN (read per call): 0 never, 1 (default) calls of >= 6 M items that the DMA kernel's barrier form
 * would rank, 2 every fp32 d=128 call with k <= 20, 3 as 2 with no user certified (test switch); n_splits must be 0 and the
 * workspace must hold the route's buffers (the full workspace of these shapes does).
 * crh_score_topk_screened: 1 if a call of this shape (arguments as crh_score_topk_route) takes the screened route, else 0;
 * crh_score_topk_route still reports the exact route the shape takes without it.
 * crh_score_topk_uncertified: the uncertified-user count of the last screened call on this workspace (synchronises `stream`;
 * for tests and measurements).
 * crh_score_topk_screen_plan: for a shape that takes the screened route, the item-range cuts of its fp16 pass and whether that
 * pass streams only the rows the candidate bitmap leaves (CRH_SCORE_SCREEN_COMPACT, read per call: 1 default, 0 keeps the masked
 * rows in the stream as zeros; results are identical either way). */
int crh_score_topk_screen_plan(int64_t n_users, int64_t n_items, size_t workspace_bytes, int has_bitmap, int* cuts, int* compact);
/* crh_score_topk_screen_ordered: 1 if a screened call of this shape streams the unmasked rows of its main range by descending
 * row norm (CRH_SCORE_SCREEN_ORDER, read per call: 1 default, 0 keeps the ascending order; results are identical either way):
 * the compaction is on, the fp16 pass is one cut and the workspace holds the sorted map.  High-norm rows raise every user's
 * threshold early, so fewer later rows cost a list insert.
 * crh_score_topk_screen_map (tests): only that map -- the ids of the unmasked items of [item_base + prefix, item_base + n_items)
 * under `bitmap` (bits of global ids; prefix a multiple of 32), ascending (ordered = 0) or as the ordered route streams them, and
 * the 16-bit norm keys along it, into device int32 buffers of n_items - prefix entries; *count = the entries that are meaningful.
 * Allocates its own buffers and synchronises `stream`. */
int crh_score_topk_screen_ordered(int64_t n_users, int64_t n_items, size_t workspace_bytes, int has_bitmap);
int crh_score_topk_screen_map(const uint32_t* bitmap, const float* item_emb, int64_t n_items, int64_t item_base, int64_t prefix,
                              int ordered, int32_t* map_out, int32_t* keys_out, int64_t* count, void* stream);
/* crh_score_topk_screen_rated_tiles: 1 if a screened call of this shape gates the rated-list lookups of its fp16 pass by
 * per-tile flags (CRH_SCORE_SCREEN_RATED_TILES, read per call: 1 default, 0 off; results are identical either way): the compaction
 * is on, the call has rated lists and the workspace holds the flags and the inverse of the streamed map.  The flags: per workgroup
 * of 512 user slots one 256-byte piece per 512 tiles of the stream, tile t of the workgroup's run in word t >> 3, nibble 4 (t & 7),
 * bit w set iff a slot of the workgroup's wave w (128 slots) rated an item whose live row lies in the tile.
 * crh_score_topk_screen_flags_bytes: bytes of the flags of n_users slots over a main range of n_main items.
 * crh_score_topk_screen_flags (tests): only those flags, over the map of crh_score_topk_screen_map with the same arguments, into
 * a device buffer of that many bytes.  Allocates its own buffers and synchronises `stream`. */
int crh_score_topk_screen_rated_tiles(int64_t n_users, int64_t n_items, size_t workspace_bytes, int has_bitmap, int has_rated);
size_t crh_score_topk_screen_flags_bytes(int64_t n_users, int64_t n_main);
int crh_score_topk_screen_flags(const uint32_t* bitmap, const float* item_emb, int64_t n_items, int64_t item_base, int64_t prefix,
                                int ordered, const int64_t* rated_rowptr, const int32_t* rated_col, int64_t n_users,
                                uint32_t* flags_out, void* stream);
int crh_score_topk_screened(int elem_bytes, int64_t n_users, int64_t n_items, int d, int k, size_t workspace_bytes,
                            int has_bitmap, int n_splits);
int64_t crh_score_topk_uncertified(const void* workspace, void* stream);
/* The screened route's PREPARED ITEMS.  Stage 0 of a screened call has an item half -- the table's scale and norm keys, the
 * live-row map under the bitmap and its sort, the packed fp16 copy with the maxima R, N, N^ of the certificate's bound, the tile
 * bits -- that depends on the item shard and the candidate bitmap alone.  An evaluation walks many user blocks against one
 * frozen table, so a caller may run that half once into a device buffer of its own and hand it to every call:
 *   crh_score_screen_items_bytes    bytes of that buffer for a shard of n_items rows, with or without a bitmap (no GPU needed);
 *   crh_score_screen_items_prepare  runs the item half on `stream` into items_buf (256-byte aligned) for calls of n_users users
 *                                   with a workspace of workspace_bytes (they decide whether the fp16 pass is compacted and
 *                                   ordered); `workspace` holds the temporaries and may be the calls' own.  *handle receives a
 *                                   small host object that records what the state was built for.  No host synchronisation;
 *   crh_score_topk_f32_prepared     crh_score_topk_f32_ex plus that handle (or NULL).  The state is used only when the call takes
 *                                   the screened route, item_emb, n_items, item_base, cand_bitmap, the prefix and `stream` are
 *                                   those it was prepared with, and the call's own compact / ordered decisions equal the
 *                                   state's; the call then runs only the user half of stage 0.  Any other call rebuilds in its
 *                                   workspace: a mismatch is not an error.  CRH_SCORE_SCREEN_PREPARED (read per call): 1
 *                                   (default) use a matching state, 0 ignore it.  Results are identical either way;
 *   crh_score_screen_items_destroy  frees the handle (not the buffer, which the caller owns);
 *   crh_score_topk_screen_item_preps  runs of the item half in this process so far, prepared or inside a call.
 * CONTRACT: the handle compares pointers, not contents.  Between prepare and the last call that uses the handle neither the
 * item rows nor the bitmap words may change, and items_buf must stay allocated and untouched; after a change, prepare again.  This
 * is a matter of soundness, not only of speed: the certificate's R, N, N^ are those of the prepared copy. */
size_t crh_score_screen_items_bytes(int64_t n_items, int has_bitmap);
int crh_score_screen_items_prepare(const float* item_emb, int64_t n_items, int d, const uint32_t* cand_bitmap, int64_t item_base,
                                   int64_t n_users, void* items_buf, size_t items_bytes, void* workspace, size_t workspace_bytes,
                                   void* stream, void** handle);
int crh_score_screen_items_destroy(void* handle);
int64_t crh_score_topk_screen_item_preps(void);
int crh_score_topk_f32_prepared(const float* user_emb, const int32_t* users, int64_t n_users,
                                const float* item_emb, int64_t n_items, int d,
                                const int64_t* rated_rowptr, const int32_t* rated_col,
                                const uint32_t* cand_bitmap, int k, int64_t item_base,
                                float* out_score, int32_t* out_idx, void* workspace,
                                size_t workspace_bytes, void* stream, int n_splits,
                                void* ev_kernel_start, void* ev_kernel_stop, const void* prepared);
int crh_score_topk_f32(const float* user_emb, const int32_t* users, int64_t n_users,
                       const float* item_emb, int64_t n_items, int d,
                       const int64_t* rated_rowptr, const int32_t* rated_col,
                       const uint32_t* cand_bitmap, int k, int64_t item_base,
                       float* out_score, int32_t* out_idx,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Tuning / test / measurement hook: same as above with the item-range split count forced
 * (0 = automatic; results are identical for every split count, canonical merge) and two
 * optional hipEvent_t (as void*, may be NULL) recorded on `stream` immediately before and
 * after the scoring kernel itself, so a caller can time that kernel apart from the merge. */
int crh_score_topk_f32_ex(const float* user_emb, const int32_t* users, int64_t n_users,
                          const float* item_emb, int64_t n_items, int d,
                          const int64_t* rated_rowptr, const int32_t* rated_col,
                          const uint32_t* cand_bitmap, int k, int64_t item_base,
                          float* out_score, int32_t* out_idx,
                          void* workspace, size_t workspace_bytes, void* stream, int n_splits,
                          void* ev_kernel_start, void* ev_kernel_stop);

/*
 * fp16 variant for generated embeddings (SURVEY.md 8(f)3 / BASELINE.json configs[4]: model/DropoutNet.py:126-135
 * produces the tables, :67-72 scores them with the same user_emb[users] @ item_emb.T).  Tables are IEEE half,
 * row-major, d in {16,32,64,128,256}; products are exact in fp32 and accumulated in fp32 by
 * v_mfma_f32_32x32x16_f16 (the accumulation order inside one 16-wide MFMA step is the hardware's, so
 * scores are compared with a tolerance, not bit for bit; the ORDER of the returned list is canonical for
 * the scores the kernel computed).  Masks, splits, workspace protocol, events: as crh_score_topk_f32_ex.
 */
int crh_score_topk_f16_supports_dim(int d);
size_t crh_score_topk_f16_workspace_bytes(int64_t n_users, int64_t n_items, int d, int k);
int crh_score_topk_f16_ex(const void* user_emb, const int32_t* users, int64_t n_users,
                          const void* item_emb, int64_t n_items, int d,
                          const int64_t* rated_rowptr, const int32_t* rated_col,
                          const uint32_t* cand_bitmap, int k, int64_t item_base,
                          float* out_score, int32_t* out_idx,
                          void* workspace, size_t workspace_bytes, void* stream, int n_splits,
                          void* ev_kernel_start, void* ev_kernel_stop);

/*
 * Mask + top-k over an already materialised dense score block (any batch_predict, e.g.
 * model/VBPR.py:68-75, model/ALDI.py:149-160): model/BaseRecommender.py:175-183.
 * scores (n_users, row_stride) fp32; masked entries are also written back as -1e9 when
 * write_back != 0 (the reference mutates the block in place).
 */
int crh_mask_topk_f32(float* scores, int64_t n_users, int64_t n_items, int64_t row_stride,
                      const int64_t* rated_rowptr, const int32_t* rated_col,
                      const uint32_t* cand_bitmap, int k, int64_t item_base, int write_back,
                      float* out_score, int32_t* out_idx, void* stream);

/*
 * Canonical merge of n_lists partial top-k lists per user, layout [list][user][k_in]
 * (item-range splits inside one GPU; shards after the all-gather).
 * n_lists <= 64, k_in, k_out <= CRH_MAX_K (the reference takes any --topN, model/BaseRecommender.py:27-29; lists of
 * up to 128 entries are kept two per lane).
 */
int crh_merge_topk(const float* in_score, const int32_t* in_idx, int n_lists, int64_t n_users,
                   int k_in, int k_out, float* out_score, int32_t* out_idx, void* stream);

/*
 * One BPR training step's loss + gradients (everything but the optimiser).
 * Replaces model/MF.py:21-26 / model/LightGCN.py:23-27:
 *     u, p, n = user_tab[user_idx], pos_tab[pos_idx], neg_tab[neg_idx]        (list-index gather)
 *     loss    = bpr_loss(u,p,n) + l2_reg_loss(reg,u,p,n)      util/utils.py:25-29,44-48
 *     loss.backward()      (index backward = index_put_(accumulate=True) into dense gradients)
 * tables (rows, d) fp32, d % 4 == 0, 16-byte aligned; *_idx (batch) int32 or NULL (= rows 0..batch-1,
 * i.e. the tensors are already gathered: this is then bpr_loss/l2_reg_loss on (B,d) tensors).
 * grad_* are dense tables the gradients are ACCUMULATED into (zero them first; pos and neg may be the
 * same table); pass all three NULL for forward only.  loss_out[0] = bpr, loss_out[1] = l2 (device).
 * plan (device int32, or NULL): the batch's reverse index -- [nu, ni, L, user rows[L], offsets[L+1],
 * triple ids[L], item rows[2L], offsets[2L+1], entries[2L] = b | role<<30, n_heavy, heavy slots[3L/T+2]], T = crh_bpr_heavy_threshold(),
 * L >= batch the layout size; a heavy slot names a row with more than T entries (r < nu: user row r, else item
 * row r - nu), ascending -- built by crh_bpr_plan_build_host or on the device (crh_bpr_plan_build).  With a
 * plan every touched gradient row is summed in a fixed order (by one lane group; a heavy row by one workgroup, in
 * the same launch) and STORED (deterministic, no atomics; rows not touched are left as they are, i.e. zero);
 * it requires pos_table == neg_table and grad_pos == grad_neg.  Without a plan rows are accumulated
 * with fp32 atomics.
 */
size_t crh_bpr_workspace_bytes(int64_t batch);
int64_t crh_bpr_plan_ints(int64_t batch);
int crh_bpr_heavy_threshold(void);   /* a row with more entries than this is on the plan's heavy list */
int crh_bpr_plan_build_host(const int32_t* user_idx_host, const int32_t* pos_idx_host,
                            const int32_t* neg_idx_host, int64_t batch, int64_t layout_batch,
                            int32_t* plan_out_host);   /* crh_bpr_plan_ints(layout_batch) ints */
/* Device version: the plans of all ceil(n_records / batch_size) batches of an epoch in one launch
 * (LDS bitonic sort per batch; batch_size <= 8192).  plans_out: n_batches * crh_bpr_plan_ints(batch_size). */
int crh_bpr_plan_build(const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                       int64_t n_records, int64_t batch_size, int32_t* plans_out, void* stream);
/* Same plans for ANY batch size up to 524 288 (S-TRAIN-XL: 65 536): several workgroups per batch -- chunk sorts in LDS,
 * merge-path passes in global memory, segment emission, heavy lists -- a handful of launches for all batches of the
 * call.  Bit-identical to crh_bpr_plan_build where both apply.  Workspace: crh_bpr_plan_build_large_workspace_bytes. */
size_t crh_bpr_plan_build_large_workspace_bytes(int64_t n_records, int64_t batch_size);
int crh_bpr_plan_build_large(const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                             int64_t n_records, int64_t batch_size, int32_t* plans_out, void* workspace,
                             size_t workspace_bytes, void* stream);
int crh_bpr_fwd_bwd_f32(const float* user_table, const float* pos_table, const float* neg_table, int d,
                        const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx,
                        int64_t batch, float reg, float* grad_user, float* grad_pos, float* grad_neg,
                        float* loss_out, const int32_t* plan, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * The same step split for data-parallel training (the batch is sharded over the ranks,
 * tables replicated).  l2_reg_loss (util/utils.py:44-48) uses the Frobenius norm of the WHOLE gathered
 * batch and bpr_loss (util/utils.py:25-29) its mean, so the backward pass of a slice needs four sums over
 * all slices.  crh_bpr_fwd_f32 runs the forward over this rank's `batch` triples and leaves
 * sums_out[4] = {sum u^2, sum p^2, sum n^2, sum -log(1e-5+sigmoid(x))} (device); the caller all-reduces
 * them (RCCL, 16 bytes); crh_bpr_bwd_f32 then accumulates / stores this slice's gradient rows using the
 * global sums and `global_batch`, and writes loss_out = the GLOBAL [bpr, l2].  `workspace` must be the
 * buffer the forward of the same slice used (it carries the per-triple score differences).
 */
int crh_bpr_fwd_f32(const float* user_table, const float* pos_table, const float* neg_table, int d,
                    const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx, int64_t batch,
                    float* sums_out, void* workspace, size_t workspace_bytes, void* stream);
int crh_bpr_bwd_f32(const float* user_table, const float* pos_table, const float* neg_table, int d,
                    const int32_t* user_idx, const int32_t* pos_idx, const int32_t* neg_idx, int64_t batch,
                    int64_t global_batch, float reg, const float* sums, float* grad_user, float* grad_pos,
                    float* grad_neg, float* loss_out, const int32_t* plan, void* workspace,
                    size_t workspace_bytes, void* stream);

/*
 * Row-ownership split of the same backward, for the data-parallel TOUCHED-ROWS step (SURVEY.md 8(e), S-TRAIN-XL: the
 * dense gradient all-reduce of the split above is 5.6 GB per step there).  Every rank holds the whole batch, its plan,
 * the forward of the whole batch (crh_bpr_fwd_f32 over `workspace`) and its `sums`; rank r computes only the gradient rows
 * of the plan's row slots w with w % own_mod == own_rem -- each row summed by ONE rank in the plan's entry order, i.e. the
 * bits of the single-GPU launch of model/MF.py:22-26's backward.  The ranks then exchange whole rows: crh_rows_pack_f32
 * gathers the owned rows of the gradient table into crh_rows_pack_cap(batch, own_mod) slots of (row id, d floats) (ids past
 * the plan's rows: -1), one all-gather moves them, crh_rows_unpack_f32 STORES every rank's rows into the gradient table
 * (each row has exactly one owner: nothing is added), and crh_adam_rows_f32 runs over the whole plan on every replica.
 * item_table is the shared positive / negative table (a plan requires it); d <= 256.
 */
int crh_bpr_bwd_owned_f32(const float* user_table, const float* item_table, int d, const int32_t* user_idx,
                          const int32_t* pos_idx, const int32_t* neg_idx, int64_t batch, float reg, const float* sums,
                          float* grad_user, float* grad_item, float* loss_out, const int32_t* plan, int own_mod,
                          int own_rem, void* workspace, size_t workspace_bytes, void* stream);
int64_t crh_rows_pack_cap(int64_t batch, int own_mod);
int crh_rows_pack_f32(const float* table, const int32_t* plan, int64_t batch, int64_t user_rows, int d, int own_mod,
                      int own_rem, int32_t* out_ids, float* out_rows, void* stream);
int crh_rows_unpack_f32(float* table, const int32_t* ids, const float* rows, int64_t n, int d, void* stream);

/*
 * torch.optim.Adam(lr) defaults, dense, for up to two tensors in one launch (model/MF.py:14,27:
 * user table then item table, equal step counters).  Mirrors torch/optim/adam.py
 * _single_tensor_adam op for op; scalar factors are evaluated in double.  step starts at 1.
 * zero_grad != 0 also clears g (the next optimizer.zero_grad()).  n0, n1 multiples of 4; n1 may be 0.
 * step_scalars (device, 2 floats, or NULL): when given, the step-dependent factors
 * {sqrt(1-beta2^step), -lr/(1-beta1^step)} are read from memory instead of being derived from
 * `step`, so that a captured hipGraph of an epoch can be replayed with fresh values
 * (crh_adam_step_scalars_host computes them on the host).
 */
int crh_adam_dense_f32(float* p0, float* g0, float* m0, float* v0, int64_t n0,
                       float* p1, float* g1, float* m1, float* v1, int64_t n1,
                       double lr, double beta1, double beta2, double eps, int64_t step, int zero_grad,
                       const float* step_scalars, void* stream);
void crh_adam_step_scalars_host(double lr, double beta1, double beta2, int64_t step, float* out2_host);
void crh_adam_step_scalars_range_host(double lr, double beta1, double beta2, int64_t first_step, int64_t n,
                                      float* out_host);   /* n pairs, steps first_step .. first_step+n-1 */

/*
 * Touched-rows replay of the same dense Adam, for tables whose gradient is zero in almost every row (BPR-MF at
 * catalogue scale: SURVEY.md 8(d) S-TRAIN-XL touches 196 K of 11 M rows per step, and the dense pass is 99.5 % of
 * the step's HBM traffic).  Rows are independent and the update is elementwise, so a row that was not touched
 * between steps s and t is brought up to date later by replaying its zero-gradient steps s+1..t-1 in registers:
 * the same fp32 operations in the same order as crh_adam_dense_f32, hence the same bits.
 *   p, g, m, v   (n_rows, d) fp32 tables (users first); last_step (n_rows) int32, zero-initialised
 *   plan         the batch's reverse index (crh_bpr_plan_build*); its item rows are offset by user_rows
 *   scalar_table device floats [2 * (max_step + 1)]: entry s = crh_adam_step_scalars_host(lr, b1, b2, s)
 *   mode 0  catch-up: rows of the plan become valid for step-1   (before the forward pass of `step`)
 *   mode 1  step:     rows of the plan take step `step` with g = their gradient rows, which are cleared
 *   mode 2  flush:    ALL rows become valid for `step`            (before the tables are read or saved)
 * catch-up(t) -> crh_bpr_fwd_bwd_f32(plan) -> step(t) for t = 1, 2, ..., then flush(T), equals T dense steps.
 */
int crh_adam_rows_f32(float* p, float* g, float* m, float* v, int32_t* last_step, int64_t n_rows, int d,
                      const int32_t* plan, int64_t batch, int64_t user_rows, int64_t step,
                      const float* scalar_table, double beta1, double beta2, double eps, int mode, void* stream);

/*
 * CSR SpMM with the LightGCN layer sum fused (model/LightGCN.py:88-93 and its autograd):
 *     P = A * x ;  y = P (if y) ;  acc_out = (acc_in * s_in + P) * s_out (if acc_out; acc_in NULL = 0)
 * rowptr (n_rows+1) int64, col int32 ascending per row, val fp32 (util/databuilder.py:220-254,953-962
 * produce exactly this matrix, as COO); x, y, acc_* are (n_rows, d) fp32, d % 4 == 0.
 * acc_out may alias acc_in; outputs must not alias x.
 * sched (HOST struct of DEVICE pointers, or NULL): optional load-balancing schedule built once per
 * graph -- a list of n_seg work items, each a ROW, in any order (the host mirror orders them by descending
 * length so that the lane groups of a wave walk rows of similar length):
 *     seg_row[w] = the row; seg_slot[w] = -1: finished by one lane group, bit-identical to the edge-order fma
 *     chain; >= 0: the row is "heavy" (more than crh_spmm_segment_edges() edges) and skipped here;
 *     seg_ptr: not read (kept for layout compatibility, must be non-NULL);
 *     multi_row[m], m < n_multi: the heavy WORKGROUPS, which lead the grid (list the longest rows first) -- a heavy
 *     row is given to a whole workgroup whose lane groups split its edge list and combine their partial sums in a
 *     fixed order (deterministic; the association differs from the single chain);
 *     multi_count[m] = n_sub | sub << 8 (NULL = 1 everywhere): n_sub in {1, 2, 4} cuts the row's column slice into
 *     n_sub ranges, workgroup `sub` taking one of them with 1 / n_sub of the lanes per lane group (n_sub times the
 *     lane groups per row: for the few rows of thousands of edges that set a launch's critical path); a row with
 *     n_sub > 1 is listed n_sub times, sub = 0 .. n_sub - 1;
 *     multi_first / n_partial: not read; nnz = number of stored edges.
 * With a schedule, and when the dense operand is larger than one XCD's L2 but a half / quarter of its columns
 * is not (and the edge list is small against it), the feature columns are processed in 2 / 4 slices pinned
 * to XCDs (block b -> slice (b % 8) % slices) so the random row gathers stay in that XCD's L2.
 * workspace: unused since the heavy rows are combined on chip (crh_spmm_workspace_bytes returns 0).
 * Without a schedule one lane group walks each row (bit-identical to the edge-order fma chain).
 */
#define CRH_SPMM_SLAB_BUCKETS 12
typedef struct {
    const int32_t* seg_row;
    const int64_t* seg_ptr;
    const int32_t* seg_slot;
    int64_t n_seg;
    const int32_t* multi_row;
    const int32_t* multi_first;
    const int32_t* multi_count;
    int32_t n_multi;
    int64_t n_partial;
    int64_t nnz;
    /* optional (NULL = absent): seg_desc[w] = {row, first edge, edges, slot} as four int32 -- the work item, its edge
     * range and its class in ONE 16-byte load instead of three dependent ones (needs nnz < 2^31) */
    const int32_t* seg_desc;
    /* optional (NULL = absent), round 3: the light rows as a STREAM of 8-byte pairs in work-item order.  Record of a row
     * with cnt edges: pair 0 = {row, cnt}, pairs 1.. = {col, fp32 bits of val} in edge order, padded with {0, 0} to
     * `units` units of slab_lanes pairs (units = 1 for cnt <= slab_lanes - 1, else 1 + ceil((cnt - (slab_lanes - 1)) /
     * slab_lanes)).  Work items are ordered by descending length, so the records of one unit count are contiguous
     * ("bucket" b: work items slab_first[b] .. slab_first[b + 1] - 1, units slab_units[b], first pair slab_base[b]) and
     * the address of a record is arithmetic: the dependent chain of a row is {record} -> {gathers} -> {store} instead of
     * {descriptor} -> {edge list} -> {gathers} -> ...  Used when slab_lanes equals the launch's lanes per lane group
     * (crh_spmm_lane_group); the stream must be followed by 2 * slab_lanes readable pairs.  n_slab = light work items. */
    const void* slab;
    int32_t slab_lanes;
    int32_t slab_buckets;
    int64_t n_slab;
    int32_t slab_first[CRH_SPMM_SLAB_BUCKETS];
    int32_t slab_units[CRH_SPMM_SLAB_BUCKETS];
    int64_t slab_base[CRH_SPMM_SLAB_BUCKETS];
    /* layout version of THIS struct, CRH_SPMM_SCHED_VERSION: the meaning of multi_count changed in round 3 (segments per
     * heavy row -> n_sub | sub << 8 per heavy workgroup) and the struct grew; a schedule built for another layout is
     * refused (CRH_ERR_ARG) instead of being decoded as something else.  multi_count entries must have n_sub in {1, 2, 4}
     * and sub < n_sub (checked by the builder, coldrec_amd/ops.py SpmmSchedule). */
    int32_t version;
} crh_spmm_sched;
#define CRH_SPMM_SCHED_VERSION 4
int crh_spmm_segment_edges(void);
/* lanes per lane group (16 bytes of a row each) the SpMM launches use for an n_rows x d operand and nnz stored edges under
 * a schedule: d / 4 / (column slices), a power of two -- what a caller needs to lay out crh_spmm_sched::slab */
int crh_spmm_lane_group(int64_t n_rows, int d, int64_t nnz);
size_t crh_spmm_workspace_bytes(const crh_spmm_sched* sched, int d);
int crh_spmm_csr_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                     const float* x, int d, float* y, const float* acc_in, float s_in,
                     float* acc_out, float s_out, const crh_spmm_sched* sched, void* workspace,
                     size_t workspace_bytes, void* stream);

/*
 * The last SpMM of LightGCN's backward pass with torch.optim.Adam fused into its epilogue (model/LightGCN.py:26-28):
 * g = (acc_in * s_in + A x) * s_out is the gradient of the embedding table p (also stored to acc_out if not NULL);
 * one Adam step with crh_adam_dense_f32's arithmetic (same bits) on (p, m, v) in place; zero_acc_in != 0 clears
 * acc_in's row after it was consumed (ready for the next step's gradient scatter; acc_in must then differ from x).
 */
int crh_spmm_csr_adam_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                          const float* x, int d, float* acc_in, float s_in, float* acc_out, float s_out,
                          const crh_spmm_sched* sched, float* p, float* m, float* v, double lr,
                          double beta1, double beta2, double eps, int64_t step,
                          const float* step_scalars, int zero_acc_in, void* stream);

/*
 * One optimiser step of model/MF.py:19-27 (gather, bpr_loss + l2_reg_loss, backward, torch.optim.Adam) in ONE
 * launch, for tables that live in cache (MovieLens / CiteULike scale) where a step is launch and memory latency.
 * Organised by table row: each row's gradient is summed in plan-list order (score differences recomputed from the
 * rows, no forward pass, no gradient table), Adam is applied in registers and the new row goes to the OTHER
 * parameter buffer (table_in != table_out; m, v in place).  The Frobenius norms a step needs are produced by
 * the PREVIOUS call from the rows it has just updated (multiplicity in the next batch x |row|^2), as partial sums:
 *   part_in   [n_parts_in][4]: (sum u^2, sum p^2, sum n^2) of THIS batch and the loss sum of the PREVIOUS one;
 *             from the previous call's part_out (n_parts_in = crh_mf_step_parts(rows, d)) or, for the first step
 *             of an epoch, the first crh_bpr_fwd_parts(batch, d) x 4 floats of crh_bpr_fwd_f32's workspace
 *   part_out  [crh_mf_step_parts][4]
 *   crh_mf_step_tables flattens an epoch's plans once: range (n_batches, rows) int2 = the row's slice of the
 *             batch's entries, (0,0) if untouched; entries (n_batches, 3*batch_size) int2 = the two other rows of
 *             the triple (table rows, users first; role << 30 in .x on the item side); mult (n_batches, rows) =
 *             multiplicities of the row in the batch (user rows: count; item rows: positives | negatives << 16)
 *   a step takes its batch's plan (heavy-row list), range and entries rows, and the NEXT batch's mult row
 *             (NULL for the last step of the epoch)
 *   loss_out[1] (l2) is written by this call; loss_out[0] (bpr) by the NEXT call through loss_prev_out
 *   (batch_prev = this call's batch) or by crh_mf_step_finish after the last step.
 *   step_scalars: device {sqrt(1-beta2^step), -lr/(1-beta1^step)} (crh_adam_step_scalars_range_host).
 * Deterministic (no atomics); equal to crh_bpr_fwd_bwd_f32(plan) + crh_adam_dense_f32 up to fp32 summation
 * order of the three norms.  d % 4 == 0, d <= 256, batch_size < 32768.
 */
int crh_bpr_fwd_parts(int64_t batch, int d);
int crh_mf_step_parts(int64_t n_rows, int d);
int crh_mf_step_tables(const int32_t* plans, const int32_t* user_idx, const int32_t* pos_idx,
                       const int32_t* neg_idx, int64_t n_records, int64_t batch_size, int64_t user_rows,
                       int64_t item_rows, int32_t* range_out, int32_t* mult_out, int32_t* entries_out,
                       void* stream);
int crh_mf_step_f32(const float* table_in, float* table_out, float* m, float* v, int64_t user_rows,
                    int64_t item_rows, int d, int64_t batch, float reg, const int32_t* plan,
                    const int32_t* range, const int32_t* entries, const int32_t* mult_next,
                    const float* part_in, int n_parts_in, float* part_out, float* loss_prev_out,
                    int64_t batch_prev, float* loss_out, double beta1, double beta2, double eps,
                    const float* step_scalars, void* stream);
int crh_mf_step_finish(const float* part_in, int n_parts_in, int64_t batch, float* loss_out, void* stream);
/*
 * north_star's "BPR loss + SGD update": torch.optim.SGD(lr) defaults (no momentum, no weight decay) in place of
 * torch.optim.Adam.  The reference itself trains with Adam (model/MF.py:14, model/LightGCN.py:16), so
 * these are the extra mode; canonical arithmetic p <- fma(-lr, g, p) (oracle/oracle_np.py sgd_dense, pinned to
 * torch.optim.SGD within fp32 rounding).  A zero gradient moves nothing, so the dense pass (crh_sgd_dense_f32, n % 4
 * == 0, zero_grad clears g), the pass over the rows of a batch's plan (crh_sgd_rows_f32: tables (rows, d), users
 * first, item rows of the plan offset by user_rows; clears the gradient rows it consumed) and the fused forms give
 * the same tables:
 *   crh_mf_step_sgd_f32   crh_mf_step_f32 without m / v / step_scalars: a row is read once and written once
 *   crh_spmm_csr_sgd_f32  crh_spmm_csr_adam_f32 with the SGD update in the epilogue
 */
int crh_sgd_dense_f32(float* p, float* g, int64_t n, double lr, int zero_grad, void* stream);
int crh_sgd_rows_f32(float* p, float* g, int d, const int32_t* plan, int64_t batch, int64_t user_rows, double lr,
                     void* stream);
int crh_mf_step_sgd_f32(const float* table_in, float* table_out, int64_t user_rows, int64_t item_rows, int d,
                        int64_t batch, float reg, const int32_t* plan, const int32_t* range, const int32_t* entries,
                        const int32_t* mult_next, const float* part_in, int n_parts_in, float* part_out,
                        float* loss_prev_out, int64_t batch_prev, float* loss_out, double lr, void* stream);
int crh_spmm_csr_sgd_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* x,
                         int d, float* acc_in, float s_in, float* acc_out, float s_out, const crh_spmm_sched* sched,
                         float* p, double lr, int zero_acc_in, void* stream);

/*
 * l2_reg_loss(reg, *embeddings) of util/utils.py:44-48 = reg * sum_e |e|_F / rows(e), for plugins that call it with
 * their own tensors (2..6 of them, any shapes): crh_l2_norm_f32 leaves |x|_F of n contiguous floats in norm_out
 * (device scalar; deterministic two-stage reduction through `workspace`, crh_l2_workspace_bytes() bytes);
 * crh_l2_reg_bwd_f32 is the backward of one term: gx (+)= x * reg * grad_out / (rows * norm), 0 where norm == 0
 * (grad_out: device scalar or NULL = 1; accumulate != 0 adds to gx).
 */
size_t crh_l2_workspace_bytes(void);
int crh_l2_norm_f32(const float* x, int64_t n, float* norm_out, void* workspace, size_t workspace_bytes, void* stream);
int crh_l2_reg_bwd_f32(const float* x, int64_t n, int64_t rows, float reg, const float* norm, const float* grad_out,
                       float* gx, int accumulate, void* stream);

/*
 * Multi-GPU exchange steps over RCCL (the reference is single-process, nothing to cite): one
 * communicator per process / GPU.  crh_comm_unique_id (rank 0; 128 bytes, hand them to the other ranks out of band)
 * -> crh_comm_init on every rank (collective) -> the two collectives below, asynchronous on `stream` -> destroy.
 *   crh_comm_allgather_topk  every rank's (n_users, k) shard lists -> gathered_* laid out [rank][user][k], which is
 *                            crh_merge_topk's input with n_lists = world (eval over a row-sharded item table).  ONE
 *                            collective: scores and ids travel packed as (n_users, 2k) 32-bit words (the layout
 *                            coldrec_amd/eval.py sends through torch.distributed) through the caller's device
 *                            `workspace` of crh_comm_allgather_topk_workspace_bytes(world, n_users, k) bytes
 *   crh_comm_allreduce_f32   in-place sum of n floats: the 4 batch sums of crh_bpr_fwd_f32, the dense gradient table
 *   crh_comm_allgather_rows  every rank's crh_rows_pack_cap slots of (row id, d floats) -> gathered_* laid out [rank][slot],
 *                            crh_rows_unpack_f32's input with n = world * cap (the touched-rows step over the ranks)
 * librccl.so is dlopen'ed on first use (an already loaded copy is reused); single-GPU callers never load it.
 * coldrec_amd's Python host layer issues the same collectives through torch.distributed ("nccl" = RCCL).
 */
typedef struct crh_comm crh_comm;
int crh_comm_unique_id(void* id128_host);
crh_comm* crh_comm_init(int rank, int world, const void* id128_host);
int crh_comm_destroy(crh_comm* c);
int crh_comm_rank(const crh_comm* c);
int crh_comm_world(const crh_comm* c);
int crh_comm_allreduce_f32(crh_comm* c, float* buf, int64_t n, void* stream);
int crh_comm_allgather_rows(crh_comm* c, const int32_t* ids, const float* rows, int64_t cap, int d, int32_t* gathered_ids,
                            float* gathered_rows, void* stream);
size_t crh_comm_allgather_topk_workspace_bytes(int world, int64_t n_users, int k);
int crh_comm_allgather_topk(crh_comm* c, const float* score, const int32_t* idx, int64_t n_users, int k,
                            float* gathered_score, int32_t* gathered_idx, void* workspace, size_t workspace_bytes,
                            void* stream);

/*
 * InfoNCE of the graph-contrastive models, forward and backward in one call (reference util/utils.py:61-76, called twice
 * per batch by model/SimGCL.py:58-59 and model/XSimGCL.py:61-62, and by model/NCL.py:61,64):
 *     Z1, Z2 = F.normalize(view1), F.normalize(view2)   (b_cos != 0; b_cos = 0 keeps the raw rows)
 *     S = Z1 Z2^T / tau;  loss = -mean(diag(log_softmax(S, 1)))
 * without the N x N matrix: two streaming passes over 32 x 32 tiles on v_mfma_f32_32x32x2_f32 (exact fp32), the row
 * pass with an online max / sum; every reduction in a fixed order (two identical calls give identical bits).
 *   view1 / view2  fp32 row-major, width d (d % 4 == 0, 4 <= d <= 256); rows1 / rows2 = int32 row ids into them (the batch
 *                  is view[rows[0..N)]; ids must be unique: gradient rows are scattered back to them), NULL = rows 0..N-1
 *   n_dev          device int32 N (clamped to [0, n_max]), NULL = n_max; grids are sized from n_max, so a step that
 *                  computes N on the device needs no host sync
 *   grad1 / grad2  d loss/d view * scale, at the rows of rows1 / rows2 (or rows 0..N-1); accumulate != 0 adds into them,
 *                  else those rows are overwritten; no other row is touched.  The normalize backward clamps the norm at
 *                  1e-12 as torch does (a zero row gets grad / 1e-12).  Either may be NULL (not computed: a NULL grad2
 *                  skips the column pass); at least one of grad1, grad2, loss_out must be given
 *   loss_out       device scalar (the unscaled mean), NULL = not written; N = 0 gives 0 and touches no gradient row
 *   workspace      crh_infonce_workspace_bytes(n_max, d) bytes, 256-byte aligned: zero-padded normalised copies of both
 *                  views (ceil32(n_max) x ceil32(d) each) plus crh_infonce_splits(n_max) partial tiles of the same size
 */
size_t crh_infonce_workspace_bytes(int64_t n_max, int d);
int crh_infonce_splits(int64_t n_max);
int crh_infonce_f32(const float* view1, const int32_t* rows1, const float* view2, const int32_t* rows2,
                    const int32_t* n_dev, int64_t n_max, int d, float tau, int b_cos, float scale, int accumulate,
                    float* grad1, float* grad2, float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The structure contrast of NCL, forward and backward in one call (reference model/NCL.py:68-94, ssl_layer_loss, called
 * twice per batch): a batch of rows against EVERY row of a table, the positive being a column of that table:
 *     X_b = F.normalize(ctx[idx_b]);  T_j = F.normalize(table[j]);  S_bj = <X_b, T_j> / tau
 *     loss = sum_b (logsumexp_{j < n_rows} S_bj - S_b,idx_b)         (a SUM over the records; the positive is inside the lse)
 * without the B x n_rows matrix: infonce's two streaming passes made rectangular (v_mfma_f32_32x32x2_f32, online max / sum in
 * the log2 domain, so the result stays finite where the reference's exp(s / tau).sum() overflows); no atomics, every
 * reduction in a fixed order (two identical calls give identical bits).
 *   ctx / table    fp32 row-major n_rows x d (d % 4 == 0, 4 <= d <= 256); may be the same pointer
 *   idx            int32 row ids of the batch, in [0, n_rows) (a precondition, NOT checked); duplicates allowed
 *   n_dev          device int32 B (clamped to [0, batch_max]), NULL = batch_max; grids are sized from batch_max
 *   grad_ctx       d loss/d ctx * scale at the batch's rows only; a row that appears c times gets the sum of its c records
 *                  (summed in ascending record order).  accumulate != 0 adds into the row, else it is overwritten
 *   grad_table     d loss/d table * scale at ALL n_rows rows (every row has a softmax term); accumulate as above
 *                  Either may be NULL (not computed: a NULL grad_table skips the column pass); at least one of grad_ctx,
 *                  grad_table, loss_out must be given.  The normalize backward clamps the norm at 1e-12 as torch does
 *   loss_out       device scalar (the unscaled sum), NULL = not written; B = 0 gives 0 and touches no gradient row
 *   workspace      crh_table_nce_workspace_bytes(batch_max, n_rows, d) bytes, 256-byte aligned: the zero-padded normalised
 *                  table (ceil32(n_rows) x ceil32(d)), the batch's copy and per-record gradients, and the split partials
 *                  of the pass that needs more -- crh_table_nce_splits(batch_max, n_rows, 0) x ceil32(batch_max) rows for
 *                  the row pass, crh_table_nce_splits(batch_max, n_rows, 1) x ceil32(n_rows) rows for the column pass (one
 *                  split once the table fills the grid): linear in n_rows, nothing of size B x n_rows
 */
size_t crh_table_nce_workspace_bytes(int64_t batch_max, int64_t n_rows, int d);
int crh_table_nce_splits(int64_t batch_max, int64_t n_rows, int col);
int crh_table_nce_f32(const float* ctx, const float* table, int64_t n_rows, const int32_t* idx, const int32_t* n_dev,
                      int64_t batch_max, int d, float tau, float scale, int accumulate, float* grad_ctx, float* grad_table,
                      float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The contrastive loss of CLCRec (reference model/CLCRec.py:117-153), forward and backward in one call.  B records, each
 * the user users[b] and 1 + G items items[b (1+G) + g] (g = 0 the positive); feat holds the content encoder's output once
 * per DISTINCT item of the batch: slot[r] = the feat row of flat row r, slot_item[s] = the item id feat row s encodes.
 *     h_b = normalize(V[it_b0])   Z_bg = normalize(F_bg)   X_bg = mix_count[bg] > 0 ? F_bg : V[it_bg]
 *     L1 = mean_b(lse_g <h_b, Z_bg>/T - <h_b, Z_b0>/T)    L2 = mean_b(lse_g <U[u_b], X_bg>/T - <U[u_b], X_b0>/T)
 *     R = (mean_b |U[u_b]| + mean_bg |V[it_bg]|) / 2      total = lr_lambda L1 + (1 - lr_lambda) L2 + reg R
 *   mix_count      int32 per flat row: how often the step's random index drew that row.  A COUNT, not a flag: the
 *                  reference assigns through an index with duplicates and autograd hands each duplicate the full
 *                  gradient, so grad_feat carries mix_count times the second softmax's term
 *   inverse indices (ops.clcrec_plan builds them): slot_rows = the flat rows grouped by slot, ascending inside a slot,
 *                  slot_ptr[n_slots + 1] their offsets; every slot's rows are cut into chunks of crh_clcrec_chunk_rows()
 *                  rows: chunk_ptr[n_slots + 1] = offsets into the chunk list, chunk_slot[n_chunks] = each chunk's slot;
 *                  user_ids[n_users] = the distinct users, user_recs = the records grouped by user (ascending inside a
 *                  user), user_ptr[n_users + 1] their offsets
 *   grad_*         d total / d table * scale, written at the touched rows only (users of the batch, items of the batch,
 *                  every feat row); any may be NULL (not computed; the others keep their bits)
 *   loss_out       4 device floats: L1, L2, R, total; NULL = not written
 *   workspace      crh_clcrec_workspace_bytes(batch, n_neg, d, n_slots) bytes, 256-byte aligned
 * d % 4 == 0, 4 <= d <= 256; 1 <= n_neg <= crh_clcrec_max_neg(); batch (1 + n_neg) < 2^31; tables and gradients 16-byte
 * aligned.  No atomics, every sum in a fixed order: two identical calls give identical bits.  One wave per record, then
 * one wave per chunk of a slot's rows, the chunks' partial sums added in chunk order; one wave per distinct user.
 */
int crh_clcrec_max_neg(void);
int crh_clcrec_chunk_rows(void);
size_t crh_clcrec_workspace_bytes(int64_t batch, int n_neg, int d, int64_t n_slots);
int crh_clcrec_f32(const float* user_table, const float* item_table, const float* feat, const int32_t* users,
                   const int32_t* items, const int32_t* slot, const int32_t* slot_item, const int32_t* mix_count,
                   const int32_t* slot_ptr, const int32_t* slot_rows, const int32_t* chunk_ptr, const int32_t* chunk_slot,
                   int64_t n_chunks, const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_recs,
                   int64_t n_users, int64_t batch, int n_neg, int d, int64_t n_slots, float temp, float lr_lambda,
                   float reg, float scale, float* grad_user, float* grad_item, float* grad_feat, float* loss_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * The loss of CCFCRec (reference model/CCFCRec.py:53-87), forward and backward in one call.  B records, each the user
 * users[b], the negative user neg_users[b] and R = 1 + P + P N + S item rows items[b R + r]: r = 0 the record's item i_b,
 * then the P positives, then the P N negatives (positive-major), then the S self-negatives; q (B, d) = the content
 * encoder's output for i_b.  With c(x) = <q_b, V[x]> / (tau |q_b| |V[x]|):
 *     L_c  = (1/P) sum_b sum_p [log(e^c(pos_bp) + sum_n e^c(neg_bpn)) - c(pos_bp)]
 *     L_s  =       sum_b       [log(e^c(i_b) + sum_s e^c(sneg_bs)) - c(i_b)]
 *     L_r1 = sum_b softplus(-(<V[i_b], U[u_b]> - <V[i_b], U[k_b]>))   L_r2 = the same with q_b in V[i_b]'s place
 *     total = lambda1 (L_c + L_s) + (1 - lambda1)(L_r1 + L_r2)           (sums over the batch, not means; no regulariser)
 * As in the reference there is no epsilon under the norms: a q row or a gathered item row of zero norm is outside the
 * contract (the result is not finite; nothing is read or written out of bounds).
 *   user_rows, item_rows  the tables' row counts; user_min .. item_max = the smallest and largest id of users + neg_users
 *                  and of items, as the caller states them (ops.ccfcrec_plan measures them): a range that leaves its
 *                  table is an argument error
 *   inverse indices (ops.ccfcrec_plan builds them): item_ids[n_items] = the distinct items, item_occ = the flat rows
 *                  b R + r grouped by item (a stable sort: ascending inside an item), item_ptr[n_items + 1] their offsets;
 *                  every item's rows are cut into chunks of crh_ccfcrec_chunk_rows(): item_chunk_ptr[n_items + 1] =
 *                  offsets into the chunk list, item_chunk_own[n_item_chunks] = each chunk's index into item_ids.  The
 *                  user_* arrays are the same over the 2B occurrences o (o < B: users[o], else neg_users[o - B])
 *   grad_user, grad_item  d total / d table * scale, written at the touched rows only (the caller zeroes the rest);
 *   grad_q         (B, d), every row.  Any may be NULL: its owner pass does not run and the others keep their bits
 *   loss_out       5 device floats: L_c, L_s, L_r1, L_r2, total; NULL = not written
 *   workspace      crh_ccfcrec_workspace_bytes(...) bytes, 256-byte aligned
 * d % 4 == 0, 4 <= d <= 256; P, N, S >= 1; R <= crh_ccfcrec_max_rows(); batch R < 2^31; tables, q and gradients 16-byte
 * aligned.  No atomics, every sum in an order fixed by the shape: two identical calls give identical bits.  One wave per
 * record, then one wave per chunk of an owner's occurrences and the chunks' partial sums added in chunk order.
 */
int crh_ccfcrec_max_rows(void);
int crh_ccfcrec_chunk_rows(void);
size_t crh_ccfcrec_workspace_bytes(int64_t batch, int n_pos, int n_neg, int n_self, int d, int64_t n_items,
                                   int64_t n_users);
int crh_ccfcrec_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                    const float* q, const int32_t* users, const int32_t* neg_users, const int32_t* items,
                    int user_min, int user_max, int item_min, int item_max,
                    const int32_t* item_ids, const int32_t* item_ptr,
                    const int32_t* item_occ, const int32_t* item_chunk_ptr, const int32_t* item_chunk_own,
                    int64_t n_items, int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr,
                    const int32_t* user_occ, const int32_t* user_chunk_ptr, const int32_t* user_chunk_own,
                    int64_t n_users, int64_t n_user_chunks, int64_t batch, int n_pos, int n_neg, int n_self, int d,
                    float tau, float lambda1, float scale, float* grad_user, float* grad_item, float* grad_q,
                    float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The loss of ALDI (reference model/ALDI.py:47-82), forward and backward in one call.  B records, each the user users[b],
 * the positive pos[b] and the negative neg[b]; the frozen teacher rows Ur = U[users[b]], Pr = V[pos[b]], Nr = V[neg[b]];
 * gen_user, gen_pos, gen_neg (B, d) = the student towers' outputs; wi = item_weight[pos[b]] (item_rows floats).  With
 * sp = <gu, gp>, sn = <gu, gn>, tp = <Ur, Pr>, tn = <Ur, Nr>, bce(x, z) = max(x, 0) - x z + log1p(exp(-|x|)) and every
 * mean over the B records:
 *     L_bpr  = mean(-log(1e-5 + sigmoid(sp - sn)))
 *     L_rate = gamma mean(|tp - sp| + |tn - sn|)                         (the derivative of |x| at 0 is 0)
 *     L_rank = alpha mean(wi bce(sp - sn, sigmoid(tp - tn)))
 *     L_iden = beta  mean(wi bce(|gp|^2 - <gp, mean_j gn_j>, sigmoid(|Pr|^2 - <Pr, mean_j Nr_j>)))
 *     total  = L_bpr + L_rate + L_rank + L_iden
 * (the reference's (gp gn^T).mean(1) is the product with the column mean; no B x B block is formed).
 *   user_rows, item_rows  the tables' row counts; user_min .. item_max = the smallest and largest id of users and of
 *                  pos + neg, as the caller states them: a range that leaves its table is an argument error (a record
 *                  whose id leaves its table all the same contributes nothing and gets zero gradient rows)
 *   grad_user, grad_pos, grad_neg  (B, d): d total / d gen_* * scale, every row.  Any may be NULL: it is neither written
 *                  nor required and the others keep their bits.  The teacher tables get no gradient
 *   loss_out       5 device floats: L_bpr, L_rate, L_rank, L_iden, total (not scaled); NULL = not written
 *   workspace      crh_aldi_workspace_bytes(batch, d) bytes (0 = a refused shape), 256-byte aligned
 * d % 4 == 0, 4 <= d <= 256; 1 <= batch < 2^31; tables, tower outputs and gradients 16-byte aligned.  No atomics, every
 * sum in an order fixed by batch and d: two identical calls give identical bits.  Five launches on the stream: the column
 * means (chunk partials, then one workgroup), one wave per record, the cross-record vector and the loss sums (one
 * workgroup), and its addition to every row of grad_neg.
 */
size_t crh_aldi_workspace_bytes(int64_t batch, int d);
int crh_aldi_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                 const int32_t* users, const int32_t* pos, const int32_t* neg, int user_min, int user_max, int item_min,
                 int item_max, const float* gen_user, const float* gen_pos, const float* gen_neg,
                 const float* item_weight, int64_t batch, int d, float alpha, float beta, float gamma, float scale,
                 float* grad_user, float* grad_pos, float* grad_neg, float* loss_out, void* workspace,
                 size_t workspace_bytes, void* stream);

/*
 * The loss of GAR (reference model/GAR.py:24-31, util/utils.py:25-48), forward and backward in one call.  B records, each
 * the user users[b], the positive pos[b] and the negative neg[b]; Ur = U[users[b]], Pr = V[pos[b]], Nr = V[neg[b]] are rows
 * of the two trained tables; gen (B, d) = the generator's output, one row per record.  With bpr(x) = -log(1e-5 +
 * sigmoid(x)), T = Pr when cold_user == 0 and Ur otherwise, and every mean over the B records:
 *     x1 = <Ur, G> - <Ur, Pr> (cold_user == 0)   x1 = <Pr, G> - <Pr, Ur> (cold_user != 0)
 *     x2 = <Ur, Pr> - <Ur, G>                    x3 = <Ur, Pr> - <Ur, Nr>
 *     L_gen = (1 - alpha) mean bpr(x1) + alpha sum |T - G|^2 / (B d)
 *     L_rec = (1 - beta) mean bpr(x2) + beta mean bpr(x3)
 *     R     = reg (|Ur|_F + |Pr|_F + |Nr|_F + |G|_F) / B       (Frobenius norms of the gathered (B, d) blocks: a duplicate
 *                                                              id counts once per occurrence; a block of zero norm
 *                                                              contributes zero gradient)
 *     total = L_gen + L_rec + R
 *   user_rows, item_rows  the tables' row counts; user_min .. item_max = the smallest and largest id of users and of
 *                  pos + neg, as the caller states them (ops.gar_plan measures them): a range that leaves its table is an
 *                  argument error
 *   inverse indices (ops.gar_plan builds them): user_ids[n_users] = the distinct users, user_occ = the records grouped by
 *                  user (a stable sort: ascending inside a user), user_ptr[n_users + 1] their offsets; every user's records
 *                  are cut into chunks of crh_gar_chunk_rows(): user_chunk_ptr[n_users + 1] = offsets into the chunk list,
 *                  user_chunk_own[n_user_chunks] = each chunk's index into user_ids.  The item_* arrays are the same over
 *                  the 2B occurrences o (o < B: pos[o], else neg[o - B]); offsets and occurrences are read as unsigned
 *   grad_user, grad_item  d total / d table * scale, written at the touched rows only (the caller zeroes the rest); an
 *                  item that is a positive and a negative, in one record or in two, receives both contributions;
 *   grad_gen       (B, d), every row.  Any may be NULL: it is not computed and the others keep their bits
 *   loss_out       4 device floats: L_gen, L_rec, R, total (not scaled); NULL = not written
 *   workspace      crh_gar_workspace_bytes(batch, d, n_items, n_users) bytes (0 = a refused shape), 256-byte aligned
 * d % 4 == 0, 4 <= d <= 256; 1 <= batch < 2^31; tables, gen and gradients 16-byte aligned.  No atomics, every sum in an
 * order fixed by the shape: two identical calls give identical bits.  One lane group per record, one workgroup for the
 * loss and the four norms, then one wave per chunk of an owner's occurrences and the chunks' partial sums added in chunk
 * order.
 */
int crh_gar_chunk_rows(void);
size_t crh_gar_workspace_bytes(int64_t batch, int d, int64_t n_items, int64_t n_users);
int crh_gar_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows, const float* gen,
                const int32_t* users, const int32_t* pos, const int32_t* neg, int user_min, int user_max, int item_min,
                int item_max, const int32_t* item_ids, const int32_t* item_ptr, const int32_t* item_occ,
                const int32_t* item_chunk_ptr, const int32_t* item_chunk_own, int64_t n_items, int64_t n_item_chunks,
                const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_occ, const int32_t* user_chunk_ptr,
                const int32_t* user_chunk_own, int64_t n_users, int64_t n_user_chunks, int64_t batch, int d, int cold_user,
                float alpha, float beta, float reg, float scale, float* grad_user, float* grad_item, float* grad_gen,
                float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * One propagation layer of NGCF (reference model/NGCF.py:94-99) over all n_rows rows, forward and backward (csrc/ngcf.hip).
 * x = x_{k-1}, s = A x (the SpMM's y), both (n_rows, d) fp32; w = [Wgc; Wbi] stacked, (2 d, d) fp32 in nn.Linear's
 * (out, in) layout; b = [bgc; bbi], (2, d), or NULL = no bias.  4 <= d <= 256, d % 4 == 0, 1 <= n_rows <= 2^30, every
 * pointer 16-byte aligned.  fp32 MFMA (exact fp32 fma chains), plain launches on `stream`, no atomics; every sum runs
 * in an order fixed by (n_rows, d), so two identical calls give identical bits.
 *
 * crh_ngcf_layer_fwd_f32:
 *     z = s Wgc^T + bgc + (x (.) s) Wbi^T + bbi ;  x_k = z > 0 ? z : 0.01 z  (z == 0 gives 0)
 *     y = x_k (if y) ;  acc_out = (acc_in * s_in + x_k) * s_out (if acc_out; acc_in NULL = 0): the SpMM's convention, so
 *     the mean over the layers costs no pass of its own.  At least one of y, acc_out must be given.
 *     acc_out may alias acc_in.  No output may alias x or s, and y must not alias acc_out.
 *
 * crh_ngcf_layer_bwd_f32: xk = x_k (only its sign is used), g = g_k = d loss / d x_k (NULL: g_k = c * dout, the top
 * layer), dout = d loss / d OUT, c = 1 / (L + 1):
 *     dz = g (.) (xk > 0 ? 1 : 0.01)                         (torch's rule: an exact zero takes 0.01)
 *     T = dz Wbi ;  ds = dz Wgc + x (.) T ;  local = c * dout + s (.) T     (g_{k-1} = local + A ds: the next SpMM's acc_in)
 *     dw = [dz^T s ; dz^T (x (.) s)]  (2 d, d), w's layout ;  db = column sums of dz  (d: the gradient of bgc AND of bbi)
 *     All four outputs are written whole.  local may alias g, and ds may alias s: a row's g and s are read for the last
 *     time before its local and ds are written.  No other output may alias an input or another output.
 *     workspace: crh_ngcf_workspace_bytes(n_rows, d) bytes, 256-byte aligned -- one (2 ceil32(d) + 1) x ceil32(d) partial
 *     of dw and db per wave of the launch (at most 2048, a function of n_rows alone) and the sums of 32 consecutive
 *     partials; a smaller one is refused with CRH_ERR_WS.
 */
size_t crh_ngcf_workspace_bytes(int64_t n_rows, int d);
int crh_ngcf_layer_fwd_f32(const float* x, const float* s, const float* w, const float* b, int64_t n_rows, int d, float* y,
                           const float* acc_in, float s_in, float* acc_out, float s_out, void* stream);
int crh_ngcf_layer_bwd_f32(const float* x, const float* s, const float* xk, const float* g, const float* dout, float c,
                           const float* w, int64_t n_rows, int d, float* ds, float* local, float* dw, float* db,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * MTPR's loss (reference model/MTPR.py:140-202), forward and backward in one call (csrc/mtpr.hip).  d = the embedding
 * width, 4 <= d <= 128, d % 4 == 0; weu, wei (2 d, d); per record b a user u, a positive i, a negative j.
 *   cold_user == 0  user_table P (user_rows, 2 d), item_table Q (item_rows, d), h (2 batch, d): row o < batch = the content
 *                   projection of the positive of record o, row batch + o of its negative
 *                   e = P[u] weu;  f_x = [Q[x] | h_x] wei,  hz_x = h_x wei[d:];  s_x = <e, f_x>,  z_x = <e, hz_x>
 *   cold_user != 0  P (user_rows, d), Q (item_rows, 2 d), h (batch, d): the content projection of the record's user
 *                   ef = [P[u] | h_b] weu,  ez = h_b weu[d:];  q_x = Q[x] wei;  s_x = <ef, q_x>,  z_x = <ez, q_x>
 *   sp(t) = softplus(-t) = max(-t, 0) + log1p(exp(-|t|)); all sums over the batch, no means:
 *     L_i = sum sp(s_i - s_j)   L_f = sum sp(z_i - z_j)   L_if = sum sp(s_i - z_j)   L_fi = sum sp(z_i - s_j)
 *     R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2)        (a row counts once per occurrence)
 *   loss_out       6 device floats: L_i, L_f, L_if, L_fi, R_emb, their sum (not scaled); NULL = not written
 *   grad_user, grad_item  d sum / d table * scale, written at the touched rows ONLY: every other row of the caller's
 *                  buffer keeps what it held (crh_adagrad_rows_f32 clears the rows it consumes, so a trainer zeroes its
 *                  buffers once); duplicate ids are summed in the plan's order
 *   grad_h, grad_weu, grad_wei  d sum / d . * scale, h's shape and (2 d, d), every element written.  Any gradient may be
 *                  NULL: it is not computed and the others keep their bits
 *   ids and inverse indices: as crh_gar_f32's, with chunks of crh_mtpr_chunk_rows() (ops.mtpr_plan builds them)
 *   workspace      crh_mtpr_workspace_bytes(batch, d, cold_user, n_items, n_users) bytes (0 = a refused shape), 256-byte
 *                  aligned: the per-record gradient rows, one (4 ceil32(d)) x ceil32(d) partial of [dweu ; dwei] per
 *                  workgroup of the tile launch (at most 512, a function of batch alone), the owner chunks' partials
 * 1 <= batch < 2^30; every float pointer 16-byte aligned.  fp32 throughout on the fp32 MFMAs; no atomics, every sum in an
 * order fixed by (batch, d) and the plan: two identical calls give identical bits.
 */
int crh_mtpr_chunk_rows(void);
size_t crh_mtpr_workspace_bytes(int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users);
int crh_mtpr_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows, const float* h,
                 const float* weu, const float* wei, const int32_t* users, const int32_t* pos, const int32_t* neg,
                 int user_min, int user_max, int item_min, int item_max, const int32_t* item_ids, const int32_t* item_ptr,
                 const int32_t* item_occ, const int32_t* item_chunk_ptr, const int32_t* item_chunk_own, int64_t n_items,
                 int64_t n_item_chunks, const int32_t* user_ids, const int32_t* user_ptr, const int32_t* user_occ,
                 const int32_t* user_chunk_ptr, const int32_t* user_chunk_own, int64_t n_users, int64_t n_user_chunks,
                 int64_t batch, int d, int cold_user, float wd1, float scale, float* grad_user, float* grad_item,
                 float* grad_h, float* grad_weu, float* grad_wei, float* loss_out, void* workspace, size_t workspace_bytes,
                 void* stream);

/*
 * The two-tower BPR loss of VBPR and AMR (reference model/VBPR.py:127-165, model/AMR.py:137-202), forward and backward in
 * one call (csrc/vbpr.hip).  d = the embedding width, 4 <= d <= 256, d % 4 == 0; per record b a user u, a positive i, a
 * negative j; user_table P (user_rows, d), item_table Q (item_rows, d); base = <P[u], Q[i] - Q[j]>.
 *   cold_user == 0  aux_table A (user_rows, d), h (2 batch, d): row o < batch = the content projection of the positive of
 *                   record o, row batch + o of its negative; h_adv = NULL or the projections of the perturbed content, h's
 *                   shape:  x = base + <A[u], h_i - h_j>,  x_adv = base + <A[u], hadv_i - hadv_j>
 *   cold_user != 0  aux_table A (item_rows, d), h (batch, d): the content projection of the record's user; h_adv must be
 *                   NULL (an argument error otherwise):  x = base + <h_b, A[i] - A[j]>
 *   sp(t) = softplus(-t) = max(-t, 0) + log1p(exp(-|t|)); all sums over the batch, no means:
 *     L_bpr = sum sp(x)    L_adv = lmd sum sp(x_adv)  (0 without h_adv)
 *     R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2 + |A[u]|^2), user mode |A[i]|^2 + |A[j]|^2 in |A[u]|^2's place
 *             (a row counts once per occurrence)
 *   loss_out       4 device floats: L_bpr, L_adv, R_emb, their sum (not scaled); NULL = not written
 *   grad_user, grad_item, grad_aux  d sum / d table * scale, written at the touched rows ONLY: every other row of the
 *                  caller's buffer keeps what it held; duplicate ids are summed in the plan's order
 *   grad_h, grad_h_adv  d sum / d . * scale, h's shape, every row written; grad_h_adv without h_adv is an argument error
 *   grad_hsum      (n_items, d) in item mode, (n_users, d) in user mode: row s = the sum of grad_h's (+ grad_h_adv's) rows
 *                  over the occurrences of the s-th distinct cold object, in the order of item_ids / user_ids -- what AMR
 *                  adds to its noise.  It does not need grad_h: it may be the only output asked for
 *                  Any output may be NULL: it is not computed and the others keep their bits; all NULL is an error
 *   ids and inverse indices: as crh_gar_f32's, with chunks of crh_vbpr_chunk_rows() (ops.vbpr_plan builds them)
 *   workspace      crh_vbpr_workspace_bytes(batch, d, cold_user, n_items, n_users) bytes (0 = a refused shape), 256-byte
 *                  aligned: the per-occurrence gradient rows, the records' terms, the owner chunks' partials
 * 1 <= batch < 2^30; every float pointer 16-byte aligned.  A record whose id leaves a table contributes nothing.  No
 * atomics, every sum in an order fixed by (batch, d) and the plan: two identical calls give identical bits.  One lane
 * group per record, one workgroup for the loss, then one wave per chunk of an owner's occurrences and the chunks'
 * partial sums added in chunk order.
 */
int crh_vbpr_chunk_rows(void);
size_t crh_vbpr_workspace_bytes(int64_t batch, int d, int cold_user, int64_t n_items, int64_t n_users);
int crh_vbpr_f32(const float* user_table, int64_t user_rows, const float* item_table, int64_t item_rows,
                 const float* aux_table, const float* h, const float* h_adv, const int32_t* users, const int32_t* pos,
                 const int32_t* neg, int user_min, int user_max, int item_min, int item_max, const int32_t* item_ids,
                 const int32_t* item_ptr, const int32_t* item_occ, const int32_t* item_chunk_ptr,
                 const int32_t* item_chunk_own, int64_t n_items, int64_t n_item_chunks, const int32_t* user_ids,
                 const int32_t* user_ptr, const int32_t* user_occ, const int32_t* user_chunk_ptr,
                 const int32_t* user_chunk_own, int64_t n_users, int64_t n_user_chunks, int64_t batch, int d, int cold_user,
                 float wd1, float lmd, float scale, float* grad_user, float* grad_item, float* grad_aux, float* grad_h,
                 float* grad_h_adv, float* grad_hsum, float* loss_out, void* workspace, size_t workspace_bytes,
                 void* stream);

/*
 * One step of DUIF (reference model/DUIF.py:19-23, util/utils.py:25-29, 44-48), forward and backward in one call
 * (csrc/duif.hip).  table T (table_rows, d): the trained table of the side without content; content C (content_rows, c)
 * fp32 row-major, 4-byte aligned only (a row starts wherever c puts it); w (d, c) = nn.Linear(c, d, bias=False).weight.
 * 4 <= d <= 256, d % 4 == 0; 1 <= c <= 4096; 1 <= batch < 2^31.  Per record b a user, a positive and a negative:
 *   cold_user == 0  u_b = T[users_b],  p_b = C[pos_b] w^T,  n_b = C[neg_b] w^T;  R = 2 batch projected rows: row o < batch
 *                   belongs to the positive of record o, row batch + o to its negative
 *   cold_user != 0  u_b = C[users_b] w^T,  p_b = T[pos_b],  n_b = T[neg_b];  R = batch projected rows
 *   x_b = <u_b, p_b - n_b>;  L_bpr = mean_b -log(1e-5 + sigmoid(x_b));  R_reg = reg (|U|_F + |P|_F + |N|_F) / batch, the
 *   Frobenius norms of the three (batch, d) blocks, duplicates counted; a norm of 0 has the gradient 0.
 *   loss_out       3 device floats: L_bpr, R_reg, their sum (not scaled); NULL = not written
 *   grad_table     d sum / d T * scale, written at the touched rows ONLY (every other row of the caller's buffer keeps what
 *                  it held); duplicate ids are summed in the plan's order
 *   grad_w         d sum / d w * scale, (d, c), every element written
 *   h_out          the projected rows H (R, d), every row written
 *                  Any output may be NULL: it is not computed and the others keep their bits; all NULL is an error
 *   free_min .. content_max: the smallest and largest id of the free side (into T) and of the projected side (into C); a
 *                  range that leaves its table is an argument error
 *   own_*          the inverse index of the FREE side's occurrences only (cold_user == 0: the batch users; else the
 *                  2 batch items, positives then negatives), as crh_gar_f32's, with chunks of crh_duif_chunk_rows()
 *                  (ops.duif_plan builds it)
 *   workspace      crh_duif_workspace_bytes(batch, d, c, cold_user, n_own) bytes (0 = a refused shape), 256-byte aligned:
 *                  H and its gradient, the free side's per-occurrence rows, the records' terms, the owner chunks' partials,
 *                  one (d, c) partial of grad_w per wave of the weight-gradient launch -- crh_duif_parts(R, d, c) of them
 *                  (0 = a refused shape), a function of the shape alone -- and the sums of crh_duif_part_chunk()
 *                  consecutive partials
 * T, w, the gradients and h_out 16-byte aligned.  fp32 throughout on the fp32 MFMAs (exact fp32 fma chains); no atomics,
 * every sum in an order fixed by (batch, d, c) and the plan: two identical calls give identical bits.  An argument error
 * returns before anything is launched.
 */
int crh_duif_chunk_rows(void);
int crh_duif_part_chunk(void);
int64_t crh_duif_parts(int64_t rows, int d, int c);
size_t crh_duif_workspace_bytes(int64_t batch, int d, int c, int cold_user, int64_t n_own);
int crh_duif_f32(const float* table, int64_t table_rows, const float* content, int64_t content_rows, int c, const float* w,
                 const int32_t* users, const int32_t* pos, const int32_t* neg, int free_min, int free_max, int content_min,
                 int content_max, const int32_t* own_ids, const int32_t* own_ptr, const int32_t* own_occ,
                 const int32_t* own_chunk_ptr, const int32_t* own_chunk_own, int64_t n_own, int64_t n_own_chunks,
                 int64_t batch, int d, int cold_user, float reg, float scale, float* grad_table, float* grad_w, float* h_out,
                 float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * torch.optim.Adagrad's defaults (lr_decay = 0, weight_decay = 0, accumulator 0) over n_ids DISTINCT rows of a (n_rows, d)
 * table, d % 4 == 0, 4 <= d <= 256 (csrc/adagrad.hip).  Per element, every operation rounded on its own:
 *     s <- s + g * g ;  p <- p + (-lr) * (g / (sqrt(s) + eps))          (lr and eps rounded to fp32)
 * then the consumed gradient rows are cleared when zero_grad != 0.  A row whose gradient is zero keeps its bits in p and
 * s, so the pass over a batch's touched rows equals the dense step.  Ids outside the table update nothing.
 */
int crh_adagrad_rows_f32(float* p, float* g, float* state_sum, const int32_t* ids, int64_t n_ids, int64_t n_rows, int d,
                         double lr, double eps, int zero_grad, void* stream);

/*
 * The loss of MetaEmbedding (reference model/MetaEmbedding.py:28-44, 168-203), forward and backward in one call
 * (csrc/metaemb.hip): a cold-start step and a warm-up step after one inner gradient step, as first-order MAML has them.
 * table (rows, d) is frozen; ids (n) point into it; emb (n, d) = the generated rows, one per occurrence; occurrence
 * i < n_pos has the target t = 1, the rest t = 0.  With o = table[ids[i]], bce(y, t) = max(y, 0) - t y +
 * log1p(exp(-|y|)), s = sigmoid and every mean over the n occurrences:
 *     y_a = <o, emb_i>                          L_a = mean bce(y_a, t)
 *     g   = (s(y_a) - t) o / n                  (a constant: the inner gradient is not differentiated)
 *     y_b = <o, emb_i - cold_lr g>              L_b = mean bce(y_b, t)
 *     ME  = alpha L_a + (1 - alpha) L_b
 *   id_min, id_max the smallest and largest id, as the caller states them: a range that leaves the table is an argument
 *                  error (an occurrence whose id leaves the table all the same contributes nothing, zero gradient row)
 *   grad_emb       (n, d): d ME / d emb * scale = scale [alpha (s(y_a) - t) + (1 - alpha) (s(y_b) - t)] o / n, every row
 *   loss_out       3 device floats: L_a, L_b, ME (not scaled)
 *   scores_out     2 n device floats: y_a of every occurrence, then y_b
 *                  Any output may be NULL: it is not written and the others keep their bits; all NULL is an error
 *   workspace      crh_metaemb_workspace_bytes(n, d) bytes (0 = a refused shape), 256-byte aligned
 * d % 4 == 0, 4 <= d <= 256; 1 <= n < 2^31; 0 <= n_pos <= n; table, emb and grad_emb 16-byte aligned.  Sigmoid and bce
 * are formed from exp(-|y|): a saturated score neither overflows nor loses the slope's sign.  No atomics, every sum in an
 * order fixed by n and d: two identical calls give identical bits.  Two launches on the stream: one lane group per
 * occurrence, then one workgroup that adds the occurrences' two terms in index order.
 */
size_t crh_metaemb_workspace_bytes(int64_t n, int d);
int crh_metaemb_f32(const float* table, int64_t rows, const int32_t* ids, int id_min, int id_max, const float* emb,
                    int64_t n, int64_t n_pos, int d, float alpha, float cold_lr, float scale, float* grad_emb,
                    float* loss_out, float* scores_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The loss of DeepMusic (reference model/DeepMusic.py:19-29, util/utils.py:32-48), forward and backward in one call
 * (csrc/deepmusic.hip).  table (rows, d) is frozen; ids (batch) point into it; gen (batch, d) = the generated rows:
 *     L_mse = sum |table[ids[b]] - gen_b|^2 / (batch d)      R = reg |gen|_F / batch      total = L_mse + R
 *   grad_gen       (batch, d): d total / d gen * scale = scale (2 (gen_b - table[ids[b]]) / (batch d) + reg gen_b /
 *                  (batch |gen|_F)), every row; the second part is zero when |gen|_F = 0.  NULL = not computed
 *   loss_out       3 device floats: L_mse, R, total (not scaled); NULL = not written; both NULL is an error
 *   id_min, id_max, workspace (crh_deepmusic_workspace_bytes(batch, d)), widths, alignment and the determinism contract
 *                  as crh_metaemb_f32's; 1 <= batch < 2^31.  Three launches: one lane group per record, one workgroup
 *                  for the loss and the norm's factor, and that factor times gen added to every row of grad_gen.
 */
size_t crh_deepmusic_workspace_bytes(int64_t batch, int d);
int crh_deepmusic_f32(const float* table, int64_t rows, const int32_t* ids, int id_min, int id_max, const float* gen,
                      int64_t batch, int d, float reg, float scale, float* grad_gen, float* loss_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/*
 * The layer perturbation of SimGCL / XSimGCL (model/SimGCL.py:106-108), in place on one (n_rows, d) fp32 layer output
 * of the propagation, d % 4 == 0, 4 <= d <= 256, every pointer 16-byte aligned.  Per row, r = the row's d uniforms:
 *     nrm = max(sqrt(sum r^2), 1e-12)                       (F.normalize's clamp)
 *     y[c] += (sign(y[c]) * (r[c] / nrm)) * eps             (sign(0) = 0: an exact zero stays zero)
 *     acc_out = (acc_in * s_in + y_new) * s_out             (only if acc_out != NULL; acc_in NULL = 0, may alias acc_out:
 *                                                            the layer mean, which must see the perturbed rows)
 * One lane group of d/4 lanes per row, the norm reduced across its lanes; no LDS, no atomics.  The uniforms:
 *   noise != NULL  read from that (n_rows, d) buffer (parity with the reference: drawn on the host by torch)
 *   noise == NULL  Philox4x32-10 in registers: key = (seed lo, seed hi), counter = (g lo, g hi, draw lo, draw hi) with
 *                  g = row * (d/4) + c/4; output word j belongs to column 4 * (c/4) + j; u = (word >> 8) * 2^-24 in [0, 1);
 *                  draw = (draw_dev ? *draw_dev : 0) + draw_offset (a device int64, so a captured graph can advance it)
 * crh_noise_uniform_f32 writes exactly the uniforms the second mode uses (the two modes compare bit for bit).
 * acc_in without acc_out is an argument error; n_rows == 0 launches nothing.
 */
int crh_noise_uniform_f32(float* out, int64_t n_rows, int d, uint64_t seed, const int64_t* draw_dev,
                          int64_t draw_offset, void* stream);
int crh_perturb_rows_f32(float* y, int64_t n_rows, int d, float eps, const float* noise, uint64_t seed,
                         const int64_t* draw_dev, int64_t draw_offset, const float* acc_in, float s_in,
                         float* acc_out, float s_out, void* stream);

/*
 * HOST-side negative sampler reproducing util/utils.py:123-157 (next_batch_pairwise) and NumPy's
 * legacy MT19937 stream bit for bit (np.random.seed / shuffle / choice), on internal ids.
 * All pointers are HOST pointers.  rec_* are the training records in file order; n_items_seen =
 * len(data.item) (negatives are drawn from every id in the item table, cold ones included).
 * crh_sampler_epoch fills one epoch (n_records triples, batches concatenated, last one short) and
 * keeps the cumulative in-place shuffle of the reference across epochs.
 * set/get_state exchange the 624-word key + position with np.random.get_state()/set_state().
 */
typedef struct crh_sampler crh_sampler;
crh_sampler* crh_sampler_create(const int32_t* rec_user_host, const int32_t* rec_item_host,
                                int64_t n_records, int32_t n_users, int32_t n_items_seen);
void crh_sampler_destroy(crh_sampler* s);
int crh_sampler_seed(crh_sampler* s, uint32_t seed);
int crh_sampler_set_state(crh_sampler* s, const uint32_t* key624_host, int pos);
int crh_sampler_get_state(const crh_sampler* s, uint32_t* key624_host, int* pos_host);
/* One epoch in the background: _async queues it for the sampler's persistent worker thread (kept spinning between
 * epochs so that its core stays at speed) and returns; _wait blocks until the epoch is complete and returns its code.
 * Between the two calls the output arrays and the sampler belong to the worker. */
int crh_sampler_epoch_async(crh_sampler* s, int64_t batch_size, int32_t* user_out_host, int32_t* pos_out_host,
                            int32_t* neg_out_host, int snapshot_first);   /* != 0: crh_sampler_snapshot on the worker first */
int crh_sampler_epoch_wait(crh_sampler* s);
/* save / bring back everything an epoch call advances (generators + cumulative permutation): speculative sampling.
 * _snapshot copies no table: the crh_sampler_epoch that follows logs the targets of its swaps and _restore replays them
 * backwards; anything else that moves the permutation under a snapshot turns it into a plain copy first.  _restore may be
 * called again after further epochs: the snapshot stays armed until the next _snapshot. */
int crh_sampler_snapshot(crh_sampler* s);
int crh_sampler_restore(crh_sampler* s);
int crh_sampler_epoch(crh_sampler* s, int64_t batch_size, int32_t* user_out_host,
                      int32_t* pos_out_host, int32_t* neg_out_host);

/*
 * The other samplers of util/utils.py, same conventions (host pointers, internal ids, one call
 * per epoch, records concatenated in shuffled order, the cumulative shuffle shared with crh_sampler_epoch).
 * They draw from CPython's `random` module stream (set/get_py_state exchange random.getstate()[1] = 624 key
 * words + position) and, where the reference does, from NumPy's (set/get_state above).
 * crh_sampler_set_catalogue must be called once first: n_users_seen = len(data.user) (pool of negative users),
 * item_is_cold[n_items_seen] = 1 for data.mapped_cold_item_idx (excluded from the CLCRec / CCFCRec candidate
 * pools), NULL = no cold item.
 *   crh_sampler_epoch_lara     util/utils.py:160-188  neg_user/neg_item: (n_records, n_negs)
 *   crh_sampler_epoch_clcrec   util/utils.py:191-233  item_out: (n_records, 1 + n_negs) = positive, then
 *                              random.sample(candidates, n_negs); sample_setsize = 21 (+ 4**ceil(log(3*n_negs, 4))
 *                              when n_negs > 5), the pool / selected-set switch of random.sample
 *   crh_sampler_epoch_ccfcrec  util/utils.py:237-300  pos_items (n, P) [NumPy stream], neg_items (n, P*N),
 *                              self_neg (n, S), neg_user (n)
 *   crh_sampler_epoch_cgrc     util/utils.py:303-336  NumPy stream only; per batch the item set in CPython's
 *                              list(set) order: bset_out[bset_ptr_out[b] .. bset_ptr_out[b+1]), n_batches + 1 offsets
 * crh_sampler_min_candidates = the smallest candidate pool over the training users (-1 before set_catalogue).
 */
int crh_sampler_set_catalogue(crh_sampler* s, int32_t n_users_seen, const uint8_t* item_is_cold_host);
int crh_sampler_set_py_state(crh_sampler* s, const uint32_t* key624_host, int pos);
int crh_sampler_get_py_state(const crh_sampler* s, uint32_t* key624_host, int* pos_host);
int64_t crh_sampler_min_candidates(const crh_sampler* s);
int crh_sampler_epoch_lara(crh_sampler* s, int32_t n_negs, int32_t* user_out_host, int32_t* item_out_host,
                           int32_t* neg_user_out_host, int32_t* neg_item_out_host);
int crh_sampler_epoch_clcrec(crh_sampler* s, int32_t n_negs, int64_t sample_setsize, int32_t* user_out_host,
                             int32_t* item_out_host);
int crh_sampler_epoch_ccfcrec(crh_sampler* s, int32_t positive_number, int32_t negative_number,
                              int32_t self_neg_number, int32_t* user_out_host, int32_t* item_out_host,
                              int32_t* neg_user_out_host, int32_t* pos_items_out_host,
                              int32_t* neg_items_out_host, int32_t* self_neg_out_host);
int crh_sampler_epoch_cgrc(crh_sampler* s, int64_t batch_size, int32_t ranking_neg_per_user,
                           int32_t* user_out_host, int32_t* item_out_host, int64_t* bset_ptr_out_host,
                           int32_t* bset_out_host, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* COLDREC_HIP_H */
