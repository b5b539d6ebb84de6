/* vidmem.h - C ABI of libvidmem.so: the MI355X (gfx950) replacement for the frame-embedding +
 * cosine/top-k hot path of VidGraph (RaphaelHaddad/Real-Time-Brain-Inspired-Video-Memory).
 *
 * The reference is pure Python and has no FFI; each entry point below names the reference call site whose
 * arithmetic it replaces (paths relative to the reference repository root).  INTEGRATION.md shows the ctypes
 * stubs a maintainer adds at those call sites.
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes.  No torch / HIP types (streams travel as void*).
 *   - every data pointer is a DEVICE pointer unless the parameter name ends in _host.
 *   - return 0 = VM_OK, negative = vm_status; text via vm_last_error(ctx).
 *   - the caller owns every buffer; the library allocates only inside vm_*_create (freed by *_destroy).
 *   - vm_preprocess / vm_encode / vm_memory_append / vm_topk_* enqueue work on the given stream and return:
 *     no hidden synchronisation, no allocation, no host threads -> capturable into a hipGraph.
 *   - calls on one handle must be stream-ordered by the caller.
 */
#ifndef VIDMEM_H
#define VIDMEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vm_ctx vm_ctx;
typedef struct vm_encoder vm_encoder;
typedef struct vm_memory vm_memory;

enum vm_status {
    VM_OK = 0,
    VM_ERR_INVALID = -1,     /* bad argument (shape / dtype / null) - the Python adapters raise on this   */
    VM_ERR_HIP = -2,         /* a HIP runtime call failed                                                */
    VM_ERR_NOMEM = -3,       /* device allocation failed or caller workspace too small                   */
    VM_ERR_UNSUPPORTED = -4, /* shape outside what the kernels are built for                             */
    VM_ERR_NO_DEVICE = -5    /* no gfx950 device visible                                                 */
};
enum vm_dtype { VM_F16 = 0, VM_BF16 = 1, VM_F32 = 2 /* vm_cosine_exact operands only */ };
enum vm_act { VM_ACT_GELU = 0, VM_ACT_QUICK_GELU = 1 };
enum vm_layout { VM_LAYOUT_CHW = 0, VM_LAYOUT_PATCHES = 1 };
/* Neo4j's vector.similarity.cosine (retriever_hybrid.py:296) is third-party and unpinned: the score mapping is
 * an explicit parameter instead of a guess.  RAW = cosine, UNIT_INTERVAL = (1 + cosine) / 2. */
enum vm_score_mode { VM_SCORE_RAW = 0, VM_SCORE_UNIT_INTERVAL = 1 };
enum vm_topk_flag { VM_FLAG_CERTIFIED = 0, VM_FLAG_GAP = 1, VM_FLAG_OVERFLOW = 3 };   /* out_query_flags values */

/* ---- context ------------------------------------------------------------------------------------------ */
int vm_init(int device, vm_ctx **out);
void vm_destroy(vm_ctx *ctx);
const char *vm_last_error(vm_ctx *ctx);
/* ABI version of this header (bumped on any signature change; 3: vm_encode_micro_batch, VM_PROF_GEMM_CLS - the arrays
 * vm_profile_read fills grew to 14 entries; 4: vm_encoder_set_option / vm_encoder_get_option replace the environment
 * variables an encoder used to read when it was created, vm_probe_mfma, vm_topk_select). */
int vm_abi_version(void);

/* ---- frame preprocessing ------------------------------------------------------------------------------
 * Replaces the CPU frame handling between cv2.VideoCapture.read and the VLM request:
 * src/pipeline/vlm_extractor.py:110-128 (BGR uint8 HWC frames; JPEG/base64 is NOT reproduced).
 * frames: uint8 [B,H,W,3] BGR.  Bilinear resize (half-pixel centres, edge clamp, no antialias) to
 * out_S x out_S, BGR->RGB, x*(1/(255*std)) - mean/std, cast to `dtype`.
 * layout CHW    : out [B,3,S,S]
 * layout PATCHES: out [B,(S/patch)^2,k_pad], k index = c*patch*patch + py*patch + px, zero-padded to k_pad
 *                 (the patch-embed GEMM's A operand; k_pad = vm_encoder_patch_k(enc)).
 * The value of one output element, every operation in fp32 and rounded once (no fused multiply-add), d = ox or oy,
 * n = W or H:   scale = (float)n / (float)out_S;  src = max(scale * (d + 0.5f) - 0.5f, 0);  i0 = min(floor(src), n - 1);
 * i1 = min(i0 + 1, n - 1);  lam = src - i0;  top = (1 - lx) * p[y0][x0] + lx * p[y0][x1], bot likewise on row y1,
 * val = (1 - ly) * top + ly * bot;  out = (dtype)(val * a + b) with a = 1.0f / (255.0f * std[c]), b = -mean[c] / std[c]
 * and the cast rounding to nearest even, subnormals kept.  oracle/frames_ref.py preprocess_ref is this expression, and
 * the output equals it bit for bit (tests/test_preprocess_gpu.py).
 * Alignment: frames may start at ANY byte address (a view into a larger buffer; frames already at out_S x out_S are read
 * in 8-byte words only when the pointer is 8-byte aligned, the result is the same either way).  out must be 16-byte
 * aligned: it is written in 16-byte pieces.
 * Returns VM_ERR_INVALID for a null ctx / frames / mean / std / out, B, H or W <= 0, a dtype other than VM_F16 / VM_BF16,
 * an unknown layout, PATCHES with patch <= 0, out_S % patch != 0, k_pad % 8 != 0 or k_pad < 3 * patch * patch, a std[c]
 * that is not > 0, or a misaligned out; VM_ERR_UNSUPPORTED for out_S <= 0 or out_S % 8 != 0.  Nothing is enqueued then. */
int vm_preprocess(vm_ctx *ctx, const uint8_t *frames_hwc_bgr, int B, int H, int W, const float mean_host[3],
                  const float std_host[3], int out_S, int dtype, int layout, int patch, int k_pad, void *out,
                  void *stream);

/* ---- vision encoder -----------------------------------------------------------------------------------
 * Replaces the remote model behind VLMExtractor._call_vlm_api (src/pipeline/vlm_extractor.py:130-185) and
 * behind OpenAIEmbeddings.aembed_query (src/components/neo4j_handler.py:27-31,333;
 * src/components/pre_llm_injector.py:207-221): frames -> one embedding vector each. */
typedef struct vm_encoder_desc {
    int image;      /* input side, 224 or 336                          */
    int patch;      /* 16 or 14                                        */
    int hidden;     /* 768 / 1024                                      */
    int layers;     /* 12 / 24                                         */
    int heads;      /* 12 / 16 (head dim must be 64)                   */
    int mlp;        /* 3072 / 4096                                     */
    int act;        /* vm_act                                          */
    int pre_ln;     /* 1: LayerNorm after the embeddings (CLIP)        */
    int patch_bias; /* 1: patch-embed conv has a bias (ViT)            */
    int proj_dim;   /* 0: none, else output projection rows            */
    int dtype;      /* vm_dtype of GEMM operands and of the output     */
    float ln_eps;
} vm_encoder_desc;

/* weights_host: array of DEVICE pointers, in this order (n = 9 + 12*layers):
 *   0 patch_w [hidden, k_pad] dtype (k = c*p*p+py*p+px, zero-padded)   1 patch_b [hidden] f32
 *   2 cls [hidden] f32        3 pos [tokens, hidden] f32
 *   4 pre_ln_g  5 pre_ln_b  (f32 [hidden]; ignored unless pre_ln)
 *   6 ln_g  7 ln_b (final LayerNorm, f32)      8 proj_w [proj_dim, hidden] dtype (ignored if proj_dim == 0)
 *   then per layer l, base = 9 + 12*l:
 *   +0 ln1_g +1 ln1_b (f32)  +2 qkv_w [3*hidden, hidden] dtype  +3 qkv_b [3*hidden] f32
 *   +4 proj_w [hidden, hidden] dtype  +5 proj_b f32  +6 ln2_g +7 ln2_b (f32)
 *   +8 fc1_w [mlp, hidden] dtype  +9 fc1_b f32  +10 fc2_w [hidden, mlp] dtype  +11 fc2_b f32
 * All matrices are row-major [out_features][in_features] (torch.nn.Linear layout).  The library copies them
 * (device-to-device) during create; the caller may free its copies afterwards. */
int vm_encoder_create(vm_ctx *ctx, const vm_encoder_desc *desc, const void *const *weights_host, int n_weights,
                      vm_encoder **out);
void vm_encoder_destroy(vm_encoder *enc);
/* Per-encoder options (ABI 4).  The release library reads NO environment variable: what a deployment may choose is
 * set here, on the handle, between calls (not while a vm_encode of this encoder is being captured or is in flight).
 * Every value of every option produces the same embeddings bit for bit (tests/test_encoder_gpu.py).
 *   VM_ENC_OPT_SCHEDULE     vm_encoder_schedule.  TWO_STREAMS: consecutive micro-batch passes of one vm_encode call
 *                           alternate between two internal streams (forked from / joined to the caller's stream inside
 *                           the call, still capturable; one workspace per stream), so that one pass's bandwidth-bound
 *                           LayerNorms run beside the other pass's matrix-bound GEMMs.  ONE_STREAM: every kernel on the
 *                           caller's stream.  AUTO (default): TWO_STREAMS for calls of two or more passes, except
 *                           while vm_profile_enable(ctx, > 0) is in force - with two streams a kernel's event
 *                           duration includes its wait for the other stream's kernels, so timing runs take one stream.
 *   VM_ENC_OPT_MICRO_BATCH  frames per pass; 0 (default) = chosen by the library (see vm_encode_micro_batch).
 *   VM_ENC_OPT_LAST_LAYER   which rows the LAST layer computes behind its keys and values: 3 (default) = the CLS rows
 *                           only (the embedding is pooled from them), 1 = CLS rows behind the attention, 0 = every row. */
enum vm_encoder_option { VM_ENC_OPT_SCHEDULE = 0, VM_ENC_OPT_MICRO_BATCH = 1, VM_ENC_OPT_LAST_LAYER = 2 };
enum vm_encoder_schedule { VM_SCHED_AUTO = 0, VM_SCHED_ONE_STREAM = 1, VM_SCHED_TWO_STREAMS = 2 };
int vm_encoder_set_option(vm_encoder *enc, int option, int value);
int vm_encoder_get_option(const vm_encoder *enc, int option);   /* negative = vm_status */
int vm_encoder_tokens(const vm_encoder *enc);    /* patches + 1                        */
int vm_encoder_patch_k(const vm_encoder *enc);   /* 3*patch*patch rounded up to 64     */
int vm_encoder_out_dim(const vm_encoder *enc);   /* proj_dim ? proj_dim : hidden       */
size_t vm_encode_workspace_bytes(const vm_encoder *enc, int B);
/* Frames vm_encode runs per pass for a call with B frames (it walks B in micro-batches: a whole number of GEMM tile
 * rounds, and - for sequences that take one attention workgroup per (frame, head) - of attention rounds).
 * vm_encode_workspace_bytes returns twice the single-pass size for calls of more than one pass unless the schedule is
 * VM_SCHED_ONE_STREAM (one workspace per internal stream); a call that is handed less runs on one stream. */
int vm_encode_micro_batch(const vm_encoder *enc, int B);
/* patches: [B, tokens-1, patch_k] dtype (vm_preprocess, PATCHES layout).  out_emb: [B, out_dim] dtype.
 * l2_normalise: divide each embedding by its L2 norm (fp32) before the cast. */
int vm_encode(vm_encoder *enc, const void *patches, int B, void *out_emb, int l2_normalise, void *workspace,
              size_t workspace_bytes, void *stream);

/* ---- text encoder -------------------------------------------------------------------------------------
 * CLIP's text transformer (ViT-L/14 family): puts a question into the joint text-image space of a CLIP image encoder
 * built with its visual projection (proj_dim > 0), the counterpart of OpenAIEmbeddings.aembed_query(query) in
 * HybridRetriever._vector_search_chunks (src/pipeline/retriever_hybrid.py:284-306).  Token + position embedding
 * (fp32) -> layers pre-LN blocks with CAUSAL attention (the vision encoder's layer code) -> final LayerNorm of each
 * sequence's pooled row -> projection (no bias) -> optional L2 -> cast.  The pooled row is the first position whose id
 * is eot_id, or 0 when there is none (transformers' rule for eos_token_id != 2).  Token ids are clamped into
 * [0, vocab) on the device; out_flags reports it. */
typedef struct vm_text_encoder vm_text_encoder;
typedef struct vm_text_encoder_desc {
    int vocab;      /* 49408                                            */
    int context;    /* 77 (at most 80)                                  */
    int hidden;     /* 768 (% 256, <= 1024)                             */
    int layers;     /* 12                                               */
    int heads;      /* 12 (head dim must be 64)                         */
    int mlp;        /* 3072                                             */
    int act;        /* vm_act                                           */
    int proj_dim;   /* 0: none, else text_projection rows (768)         */
    int eot_id;     /* 49407                                            */
    int dtype;      /* vm_dtype of GEMM operands and of the output      */
    float ln_eps;
} vm_text_encoder_desc;
/* weights_host: array of DEVICE pointers, in this order (n = 5 + 12*layers):
 *   0 tok_emb [vocab, hidden] f32   1 pos [context, hidden] f32   2 ln_final_g  3 ln_final_b (f32 [hidden])
 *   4 proj_w [proj_dim, hidden] dtype (ignored if proj_dim == 0)
 *   then per layer l, base = 5 + 12*l: the same 12 entries as vm_encoder_create's.  Copied during create. */
int vm_text_encoder_create(vm_ctx *ctx, const vm_text_encoder_desc *desc, const void *const *weights_host,
                           int n_weights, vm_text_encoder **out);
void vm_text_encoder_destroy(vm_text_encoder *enc);
int vm_text_encoder_out_dim(const vm_text_encoder *enc);   /* proj_dim ? proj_dim : hidden */
size_t vm_text_encode_workspace_bytes(const vm_text_encoder *enc, int B, int T);
/* token_ids: device int32 [B,T], 1 <= T <= context.  out_emb [B, out_dim] dtype.  out_flags: device int32 [B] or NULL,
 * per sequence bit 0 = an id was out of range (clamped), bit 1 = no eot_id (row 0 pooled).  A sequence's embedding
 * depends only on its ids up to its pooled row: not on B, T or the ids behind it.  Same conventions as vm_encode
 * (no sync, no allocation, one stream, capturable). */
int vm_text_encode(vm_text_encoder *enc, const int32_t *token_ids, int B, int T, void *out_emb, int l2_normalise,
                   int32_t *out_flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---- embedding memory ---------------------------------------------------------------------------------
 * Replaces the Chunk.embedding store: append = src/components/neo4j_handler.py:229-242
 * (MERGE ... SET c.embedding), bulk read-back = src/components/pre_llm_injector.py:390-412.
 * Rows are kept resident in HBM as [capacity, D] dtype, plus per row an exact fp64 norm and an fp32 reciprocal
 * norm.  Row id = append order (0,1,2,...).  ring=1: after `capacity` rows the oldest are overwritten; ids keep
 * counting, only the newest `capacity` ids are searchable.
 * Any finite rows are accepted.  The searches' fp32 fast path applies while every stored row's norm is 0 or lies in
 * [2^-40, 2^40] (a bf16 row can leave that interval, an fp16 row cannot); once a row outside it was appended, every
 * search of this memory is answered exactly at exhaustive cost until vm_memory_reset - erasing or overwriting the row
 * does not bring the fast path back.  Stored NaN / inf values are undefined, as in the reference. */
int vm_memory_create(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring, vm_memory **out);
void vm_memory_destroy(vm_memory *mem);
/* rows: [B, D] dtype.  *out_first_row_host (optional) receives the id of the first appended row. */
int vm_memory_append(vm_memory *mem, const void *rows, int B, int64_t *out_first_row_host, void *stream);
int64_t vm_memory_size(const vm_memory *mem);  /* rows appended so far (host mirror)                      */
int64_t vm_memory_capacity(const vm_memory *mem);
int vm_memory_dim(const vm_memory *mem);
int vm_memory_reset(vm_memory *mem, void *stream);
/* Re-read the DEVICE row counter into the host mirror and return it (negative = vm_status).  Needed after hipGraph
 * replays of vm_memory_append (they advance only the device counter), after a graph CAPTURE of it (which advanced
 * only the host mirror) and after every vm_memory_append_novel, eager or replayed (how many rows it keeps is decided on
 * the device, so it never advances the mirror).  Synchronises `stream`; not capturable.  The reference has no counterpart (its store is a
 * database, src/components/neo4j_handler.py:229-242); this is the price of the capturable append. */
int64_t vm_memory_sync(vm_memory *mem, void *stream);
const void *vm_memory_rows(const vm_memory *mem); /* device pointer to the [capacity, D] row store          */

/* ---- grouped memory -------------------------------------------------------------------------------------
 * A grouped memory carries an int64 GROUP KEY per row.  A GROUP is a maximal run of consecutive row ids with equal keys
 * (a key that comes back after other keys opens a new group): the frames of one video chunk, appended together
 * (src/pipeline/vlm_extractor.py:44-74 stores one row per frame; ids {run}_{chunk}_{i}).  In a ring, a group whose
 * oldest rows were overwritten is made of its surviving rows, also when it straddles the physical wrap.
 * vm_memory_create_grouped allocates the key column (and a group-ordinal column) beside the rows.
 * vm_memory_append_grouped: keys = device int64 [B]; the first row continues the group of the previous call when that
 *   call was also grouped and ended with the same key.  Capturable like vm_memory_append (no allocation, no sync).
 * vm_memory_append on a grouped memory makes every row its own group (key = -1 - row id; the next grouped call opens a
 *   new group); it then runs one launch more than on a plain memory.  vm_memory_reset forgets the open group.
 * vm_memory_group_keys: device pointer to the [capacity] key column (slot order, like vm_memory_rows), 0 if not grouped. */
int vm_memory_create_grouped(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring, vm_memory **out);
int vm_memory_append_grouped(vm_memory *mem, const void *rows, int B, const int64_t *keys, int64_t *out_first_row_host,
                             void *stream);
const int64_t *vm_memory_group_keys(const vm_memory *mem);

/* ---- tagged memory --------------------------------------------------------------------------------------
 * A tagged memory carries one int64 TAG per row: which video a frame came from and when, so that one memory can hold
 * many videos and a search can name the one it wants.  It replaces the per-graph predicate of the reference's two scans
 * (src/pipeline/retriever_hybrid.py:295 `MATCH (c:Chunk {graph_uuid: $graph_uuid})`,
 * src/components/pre_llm_injector.py:395-396 `WHERE c.graph_uuid = $graph_uuid`).  In a ring a row's tag lives and dies
 * with its slot.  grouped != 0: the memory also carries group keys (vm_memory_create_grouped).
 * vm_memory_append_tagged: tags = device int64 [B]; keys = device int64 [B] on a grouped memory (NULL there: every row
 *   its own group, as vm_memory_append does), NULL otherwise.  Capturable like vm_memory_append (no allocation, no
 *   sync); one launch more than on an untagged memory.
 * vm_memory_append / vm_memory_append_grouped on a tagged memory store INT64_MIN: only a scope that starts at INT64_MIN
 *   matches such a row.  On an untagged memory every call runs exactly the launches it ran before tags existed.
 * vm_memory_tags: device pointer to the [capacity] tag column (slot order, like vm_memory_rows), 0 if not tagged. */
int vm_memory_create_tagged(vm_ctx *ctx, int64_t capacity_rows, int D, int dtype, int ring, int grouped,
                            vm_memory **out);
int vm_memory_append_tagged(vm_memory *mem, const void *rows, int B, const int64_t *tags, const int64_t *keys,
                            int64_t *out_first_row_host, void *stream);
const int64_t *vm_memory_tags(const vm_memory *mem);

/* ---- novelty-gated append ------------------------------------------------------------------------------
 * Store a row only when nothing resembles it: video is redundant, and a static shot appends rows that are one vector up
 * to noise.  The reference has no counterpart (it stores one text embedding per chunk,
 * src/components/neo4j_handler.py:229-242); decisions are taken on the reference cosine of vm_topk_cosine (fp64, one
 * rounding per product and partial sum, left to right, zero-norm guard) on the 16-bit values, bit for bit.
 * rows [B, D] dtype, 1 <= B <= 4096 (VM_ERR_UNSUPPORTED above; B = 0 is a no-op that writes *out_count = 0).
 * known_scores / known_rows: what the caller already knows about each row - the best RAW cosine of rows[i] against
 * whatever part of the memory it searched and the row that reached it (< 0: nothing found) - device arrays read at
 * element i * known_stride, so column 0 of a [B, k] top-k result is passed in place; both NULL = nothing known (the gate
 * is then among the batch only); one NULL and one not is VM_ERR_INVALID.  In row order:
 *   suppressor(i) = known_rows[i]   if known_rows[i] >= 0 and known_scores[i] > threshold
 *                 = row_of[j], j the LOWEST j < i with keep[j] and cosine(rows[i], rows[j]) > threshold, if there is one
 *   keep[i]   = no suppressor           (`>` is strict, like use_min_score: a score equal to the threshold keeps the row)
 *   row_of[i] = suppressor(i), or, when kept, the id rows[i] receives: (rows before the call) + (kept rows before i)
 * The kept rows are appended in batch order exactly as vm_memory_append[_grouped|_tagged] appends that sub-batch: row
 * bytes, norms, ring slots, tags (tags NULL on a tagged memory: INT64_MIN), group keys and ordinals (keys NULL on a
 * grouped memory: every kept row its own group; a run of equal keys among the KEPT rows is one group and continues the
 * previous call's open group under vm_memory_append_grouped's rule).  tags / keys on a memory without that column:
 * VM_ERR_INVALID.  A call that keeps nothing leaves every column, the row counter and the group state untouched;
 * threshold >= 2 keeps everything; a NaN threshold is VM_ERR_INVALID.
 * With known_* = the exact top-1 of every row over the whole memory before the call, and no stored row overwritten
 * during the call, the result equals the loop "search the memory as it stands, append one row iff its best score is not
 * above the threshold".  In a ring that wraps inside the call the rule above holds as written.
 * out_keep int32 [B] (0 / 1), out_row_of int64 [B], out_count int32 [1] (kept rows of THIS call, rewritten): device,
 * each may be NULL.  No allocation, no synchronisation, no host read-back; launches are sized from B, the row counter
 * is read on the device: capturable, e.g. {vm_topk_cosine, vm_topk_redo_flagged, vm_memory_append_novel} in one graph.
 * Host mirror: the library cannot know the kept count, so vm_memory_size is NOT advanced - vm_memory_sync brings it in
 * line.  On a memory that is not a ring the call is refused with VM_ERR_NOMEM when mirror + B exceeds the capacity (the
 * worst case; the mirror must therefore be current); whatever the mirror said, no slot at or beyond the capacity is
 * written and the counter never moves past it.
 * Workspace: vm_novelty_workspace_bytes (B x 8 bytes of norms + B x ceil(B / 64) x 8 bytes of pair bits + 2 KiB). */
size_t vm_novelty_workspace_bytes(const vm_memory *mem, int B);
int vm_memory_append_novel(vm_memory *mem, const void *rows, int B, double threshold, const double *known_scores,
                           const int64_t *known_rows, int64_t known_stride, const int64_t *tags, const int64_t *keys,
                           int32_t *out_keep, int64_t *out_row_of, int32_t *out_count, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- erase: forget rows and compact the memory ------------------------------------------------------------
 * Forget rows by tag (a whole video, a time window, several of them) or by row id (a search result), and close the
 * gaps.  The reference has no counterpart (its store only ever MERGEs, src/components/neo4j_handler.py:229-242).
 * vm_memory_erase_scoped: tagged memories only (VM_ERR_INVALID otherwise).  scope_lo / scope_hi: device int64
 *   [n_scopes], n_scopes >= 1, inclusive tag ranges by vm_topk_cosine_scoped's rule; a row is erased iff its tag lies
 *   in at least one range (lo > hi matches nothing).
 * vm_memory_erase_rows: row_ids device int64 [n]; ids < 0 or >= the row count are ignored and duplicates are allowed,
 *   so a [Q, k] top-k result with its -1 padding is passed in place.  n = 0 is a no-op: only *out_erased = 0 is written.
 * Afterwards the memory holds the surviving rows in their old order, renumbered 0 .. n'-1, and every column over slots
 * [0, n_old) is bit for bit what a FRESH memory of the same kind holds after one vm_memory_append[_grouped|_tagged] of
 * the survivors with their stored tags and keys: row bytes, norms and reciprocal norms (moved, never recomputed), tags,
 * group keys, group ordinals, the group state (groups opened, last key = the last survivor's, open iff a row is left)
 * and the row counter n'.  The vacated slots [n', n_old) are zeroed in every column: forgetting means the bytes are
 * gone.  Groups follow the definition above, a maximal run of equal keys: two groups with one key that become adjacent
 * are ONE group afterwards; a group that loses rows keeps the rest.
 * Keys written by a plain append (-1 - row id) keep their VALUE: after an erase they no longer equal -1 - id, and a
 *   later plain append can write a key that a surviving row already carries (adjacent, the two would be one group).
 *   A caller that mixes plain appends and erases on a grouped memory gives its rows keys of its own.
 * out_new_row_of: device int64 [n_old] (sized for the capacity if the count is not known), old id -> new id, or -1 for
 * an erased row.  out_erased: device int64 [1], rewritten on every call.  Either may be NULL.
 * No allocation, no synchronisation, no host read-back; the row count is read on the device and launches are sized
 * from the capacity and the workspace: capturable, e.g. {vm_memory_append_tagged, vm_memory_erase_scoped,
 * vm_topk_cosine_scoped} in one graph whose window is rewritten between replays.  Launches grow with
 * capacity / segment, not with the row count.
 * Host mirror: the count is decided on the device, so vm_memory_size is NOT adjusted - vm_memory_sync brings it in
 * line, as after vm_memory_append_novel (a non-ring memory refuses appends by the mirror: sync before appending into
 * the reclaimed capacity).
 * Rings: a ring that has not wrapped (at most `capacity` rows appended) is handled like a linear memory and goes on as
 * a ring.  A ring that has wrapped is refused with VM_ERR_UNSUPPORTED by the mirror (mirror > capacity; the mirror must
 * therefore be current); whatever the mirror said, when the DEVICE count exceeds the capacity nothing is touched and
 * *out_erased = -1.
 * Workspace: vm_memory_erase_workspace_bytes(mem, segment_rows): keep flags and their prefix (5 bytes x capacity), the
 * per-chunk counts, and one SEGMENT of scratch for every column (segment_rows x (2 D + 28) bytes).  The rows move
 * segment by segment through that scratch; segment_rows = 0 names the library's default (65,536 rows, or the capacity
 * if smaller), other values are rounded up to a multiple of 256 and capped at the default.  The call derives its
 * segment from workspace_bytes - the largest multiple of 256 rows that fits, at most the default; fewer than 256 rows
 * of scratch is VM_ERR_NOMEM.  The result does not depend on the segment. */
size_t vm_memory_erase_workspace_bytes(const vm_memory *mem, int64_t segment_rows);
int vm_memory_erase_scoped(vm_memory *mem, const int64_t *scope_lo, const int64_t *scope_hi, int n_scopes,
                           int64_t *out_new_row_of, int64_t *out_erased, void *workspace, size_t workspace_bytes,
                           void *stream);
int vm_memory_erase_rows(vm_memory *mem, const int64_t *row_ids, int64_t n, int64_t *out_new_row_of,
                         int64_t *out_erased, void *workspace, size_t workspace_bytes, void *stream);

/* ---- event segmentation: group frames by content, not by fixed chunk ---------------------------------------
 * Cut the stored rows into EVENTS: maximal runs of consecutive row ids in which each frame resembles the one before it.
 * The reference has no counterpart: it cuts a video every chunk_size_seconds (src/pipeline/vlm_extractor.py:38-46) and
 * stores one text embedding per chunk (src/components/neo4j_handler.py:229-242).
 * Live rows are the ids lo .. n-1 (lo = 0, or n - capacity in a wrapped ring).  For a live row r > lo, link(r) is the
 * reference cosine of rows r-1 and r as in vm_topk_cosine - fp64 on the stored 16-bit values, one rounding per product
 * and per partial sum, left to right, the stored fp64 norms (moved, never recomputed), a zero norm gives 0.0 - bit for
 * bit; it is symmetric in its two rows.  link(lo) = 0.0.
 * Row r OPENS an event iff
 *   r == lo, or
 *   !(link(r) > threshold)   (strict, like use_min_score and the novelty gate: a link equal to the threshold opens), or
 *   on a tagged memory, with src = tag >> 40 and ms = tag & (2^40 - 1):
 *     exactly one of tag[r-1], tag[r] is INT64_MIN, or
 *     neither is INT64_MIN and src differs, or
 *     neither is INT64_MIN, max_gap_ms >= 0, and ms[r] - ms[r-1] is negative or above max_gap_ms
 *     (two INT64_MIN rows follow the score rule only).
 * max_gap_ms < 0 switches the gap rule off (the source rule stays); max_gap_ms >= 0 on an untagged memory is
 * VM_ERR_INVALID.  A NaN threshold is VM_ERR_INVALID; threshold >= 2 makes every row its own event; -inf leaves only
 * the tag rules.
 * Events are runs of consecutive row ids, as groups are: two videos appended in alternation cut each other's events at
 * every switch.  Adjacent links chain: a slow pan whose neighbours all score 0.99 can end far from where it began -
 * there is no drift guard and no cap on an event's length (long events send vm_topk_cosine_grouped to its exhaustive
 * redo, see there; the novelty gate beside it keeps static scenes short).
 * vm_memory_events: read-only, any memory (plain, grouped, tagged, ring).  out_links [n_live] (may be NULL): link(lo + i).
 *   out_event_of [n_live] (may be NULL): the 0-based event index of row lo + i.  out_first_rows [max_events]: the first
 *   row id of event e, -1 padded; NULL iff max_events == 0.  out_n_events [1]: the TOTAL number of events, also above
 *   max_events.  All device pointers.
 * vm_memory_regroup_events: rewrites the group columns, grouped memories only (VM_ERR_INVALID otherwise), so that the
 *   grouped search returns one hit per event.  from_row: device int64 [1], or NULL = the whole memory.
 *   Whole mode (from_row NULL or *from_row <= lo): for every live row, key = the row id of its event's first row,
 *     ordinal = its event index (the oldest live row's event is 0); group state: groups = the event count, last key = the
 *     last event's key, and the last event is CLOSED: a later keyed append opens a new group whatever its key, only a
 *     tail regroup extends an event.  On a linear memory the two columns over [0, n) are bit for bit what a fresh
 *     grouped memory holds after one vm_memory_append_grouped of the same rows with those keys.
 *   Tail mode (lo < *from_row < n): rows below from_row are untouched; row from_row is judged against row from_row - 1
 *     by the rule above: if it does not open an event it takes the key and ordinal of that row, whatever put them
 *     there, otherwise its key is its own id and its ordinal the previous row's plus one; the rest follows from that
 *     row.  Group state: groups = the last row's ordinal + 1, last key = the last row's key, closed.
 *     *from_row >= n touches nothing and writes *out_n_events = 0.
 *     Plain appends, each followed by a tail regroup from its first new row, leave exactly what one whole regroup
 *     leaves at the end - on a linear memory or a ring that has not wrapped, with no erase in between.  In a wrapped
 *     ring the first live event keeps the key it was formed with; a whole regroup would renumber it.
 *   out_n_events [1] (may be NULL): the events opened among the rows the call covered.
 * Both: no allocation, no synchronisation, no host read-back; the row count is read on the device and launches are sized
 * from the capacity: capturable, and a replay after an append sees the new rows.  An empty memory writes
 * *out_n_events = 0 and nothing else.  A workspace below vm_memory_events_workspace_bytes is refused with VM_ERR_NOMEM
 * before any launch.  One exact pair per row, one pass over the rows (n x D x 2 bytes); the prefix sums run over
 * separate launches, deterministic, no atomics: the result does not depend on launch geometry or workspace size.
 * Workspace: one flag byte per slot + 16 bytes per 256 slots + 256 bytes, each array rounded up to 256 bytes.
 * vm_memory_group_ordinals: device pointer to the [capacity] group-ordinal column (slot order, like
 *   vm_memory_group_keys), 0 if not grouped. */
size_t vm_memory_events_workspace_bytes(const vm_memory *mem);
int vm_memory_events(vm_memory *mem, double threshold, int64_t max_gap_ms, double *out_links, int64_t *out_event_of,
                     int64_t max_events, int64_t *out_first_rows, int64_t *out_n_events, void *workspace,
                     size_t workspace_bytes, void *stream);
int vm_memory_regroup_events(vm_memory *mem, double threshold, int64_t max_gap_ms, const int64_t *from_row,
                             int64_t *out_n_events, void *workspace, size_t workspace_bytes, void *stream);
const int64_t *vm_memory_group_ordinals(const vm_memory *mem);

/* ---- group summaries: one centroid row and one key frame per group ------------------------------------------
 * Turn every group of a grouped memory - a fixed chunk (vm_memory_append_grouped) or an event
 * (vm_memory_regroup_events) - into ONE vector and ONE frame to show for it.  The reference stores one embedding per
 * chunk (src/components/neo4j_handler.py:229-242) and searches those (src/pipeline/retriever_hybrid.py:293-306); a
 * group's normalised mean embedding is that vector, and a second memory holding these rows has the reference's shape.
 * Grouped memories only (VM_ERR_INVALID otherwise); read-only.  Live rows are the ids lo .. n-1 as in vm_memory_events.
 * Live groups are numbered in row order: G(r) = ordinal[r] - ordinal[lo]; n_groups = G(n-1) + 1.  In a wrapped ring the
 * oldest group consists of its surviving rows.
 * first_group: device int64 [1], the first group g0 of the WINDOW; NULL = 0, a negative value = 0.  The call writes the
 * groups g0 .. min(g0 + max_groups, n_groups) - 1 to the output slots 0 .. and pads the rest of max_groups.
 * out_n_groups [1] (required): always the TOTAL number of live groups.  max_groups == 0 writes only the count (the
 * other outputs may be NULL); g0 >= n_groups writes the count and the padding; an empty memory writes
 * *out_n_groups = 0 and nothing else.
 * Per group with live rows a .. b (row ids), each output device memory, each may be NULL independently:
 *   out_first_rows int64 [max_groups]: a.  out_n_rows int64: b - a + 1.  out_keys int64: the group key of row a.
 *     Padding: -1.
 *   out_centroids [max_groups, D] of the memory's dtype, zero-padded - what vm_memory_append* accepts as it stands.
 *     S_j = the fp64 sum of the stored 16-bit values x[r][j], r = a .. b strictly in row order, from 0.0, one rounding
 *     per addition.  N = sqrt(sum_j S_j * S_j): one rounding per product and per partial sum, left to right in j, then a
 *     correctly rounded square root.  N == 0 (also a group that cancels exactly): the all-zero row.  Otherwise
 *     c_j = round16(S_j / N): one correctly rounded division, then ONE round-to-nearest-even from fp64 to the dtype
 *     (never through fp32, which would round twice); subnormals and the sign of zero are kept.
 *   out_key_rows int64 [max_groups], out_key_scores double [max_groups]: the KEY FRAME, the row of the group with the
 *     highest score(r) = the reference cosine of vm_topk_cosine with the stored centroid row c as the query and row r
 *     as the stored row (fp64 on the 16-bit values, left to right; the centroid's norm = sqrt of its sum of squares;
 *     the row's norm = its STORED fp64 norm; a zero norm gives 0.0), always RAW; ties: the lowest row id.  The score
 *     is that cosine bit for bit.  Padding: -1 and 0.0.  out_key_scores without out_key_rows is allowed; with both
 *     NULL the second pass over the rows is not launched.
 * No allocation, no synchronisation, no host read-back; the row count and *first_group are read on the device and
 * launches are sized from the capacity and max_groups: capturable, and a replay after an append sees the new rows.
 * Deterministic, no atomics: a group is summed by one workgroup in row order, so the result does not depend on launch
 * geometry, workspace size, max_groups or the window a group is asked through.  Stored NaN / inf values are undefined,
 * as elsewhere; no norm domain applies (no fp32 stage, no certificate, no redo).  D above 8,192: VM_ERR_UNSUPPORTED.
 * A workspace below vm_memory_summaries_workspace_bytes is refused with VM_ERR_NOMEM before any launch.
 * Workspace, with m = min(max_groups, capacity): 256 bytes + 8 (m + 1) bytes of group bounds + 8 bytes per slot of the
 * capacity rounded up to 256 slots (scores) + 2 D m bytes (the centroids when out_centroids is NULL), each array
 * rounded up to 256 bytes. */
size_t vm_memory_summaries_workspace_bytes(const vm_memory *mem, int64_t max_groups);
int vm_memory_summaries(vm_memory *mem, const int64_t *first_group, int64_t max_groups, void *out_centroids,
                        int64_t *out_first_rows, int64_t *out_n_rows, int64_t *out_keys, int64_t *out_key_rows,
                        double *out_key_scores, int64_t *out_n_groups, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---- cosine top-k over the memory ---------------------------------------------------------------------
 * Replaces PreLLMInjector._calculate_batch_similarities + _cosine_similarity
 * (src/components/pre_llm_injector.py:346-388) and the Cypher scan of HybridRetriever._vector_search_chunks
 * (src/pipeline/retriever_hybrid.py:293-306).
 *
 * queries [Q, D] dtype.  For every query: score each stored row with the reference cosine, order by
 * (score descending, row id ascending) - Python's stable sort over memory order - and keep the first k.
 * out_scores [Q,k] are the reference's fp64 values BIT FOR BIT (sequential fp64 sums over the stored 16-bit
 * values); out_rows [Q,k] int64 row ids, -1 padded (scores 0.0 padded).
 *   global row id written = row_id * row_stride + row_offset   (row-sharded memory; use 1, 0 on one GPU)
 *   use_min_score: keep only score > min_score (after the score_mode mapping).
 * Two-stage: an fp32 MFMA scan keeps k+slack candidates per query, which are re-scored exactly.  A query whose
 * result cannot be PROVEN equal to the exhaustive answer (fp32 error bound vs the gap to the best rejected
 * row) is counted in *out_uncertified (device int32, accumulates, may be NULL) and marked in
 * out_query_flags[q] != 0 (device int32 [Q], rewritten for every query on every call, may be NULL; the value says
 * why, vm_topk_flag: VM_FLAG_GAP = the exact k-th score does not clear the best rejected fp32 score by the error
 * bound 2 (D + 8) 2^-24 - near-ties between rank k and rank k + slack, e.g. more than `slack` exact duplicates;
 * VM_FLAG_OVERFLOW = more candidates at or above a query's cut than its buffer holds).  Pass the flags
 * to vm_topk_redo_flagged on the same stream: the reference always returns the exhaustive answer
 * (src/components/pre_llm_injector.py:356-370), so the pair {vm_topk_cosine, vm_topk_redo_flagged} is the drop-in.
 * Domain: the bound holds while the query's norm and every stored row's norm are 0 or lie in [2^-40, 2^40] (D <= 2048;
 * vm_memory_create).  Outside it every query concerned is flagged VM_FLAG_GAP and vm_topk_redo_flagged answers it: exact,
 * at exhaustive cost.  Stored NaN / inf values are undefined, as in the reference. */
size_t vm_topk_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine(vm_memory *mem, const void *queries, int Q, int k, int use_min_score, double min_score,
                   int score_mode, int64_t row_stride, int64_t row_offset, double *out_scores,
                   int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                   size_t workspace_bytes, void *stream);
/* Exhaustive fp64 redo of the flagged queries only (query_flags: device int32 [Q], as written by vm_topk_cosine):
 * their rows of out_scores / out_rows are overwritten with the exhaustive answer under the same contract; the
 * other queries are left untouched.  Row count and flags are read on the device: no host read-back, no
 * allocation, capturable into a hipGraph, and two near-empty launches when nothing is flagged.  k <= 64.
 * Workspace: vm_topk_redo_workspace_bytes (slice winners, 16 bytes x blocks x Q x k; a few MB). */
size_t vm_topk_redo_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_redo_flagged(vm_memory *mem, const void *queries, int Q, int k, int use_min_score, double min_score,
                         int score_mode, int64_t row_stride, int64_t row_offset, const int32_t *query_flags,
                         double *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                         void *stream);
/* Exhaustive fp64 version of the same contract for ALL queries (every pair scored exactly; slow, always exact;
 * workspace Q x rows x 8 bytes; sizes its grid from the host row count, so not for graph replay). */
size_t vm_topk_exact_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_exact(vm_memory *mem, const void *queries, int Q, int k, int use_min_score,
                         double min_score, int score_mode, int64_t row_stride, int64_t row_offset,
                         double *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes,
                         void *stream);
/* Grouped top-k: the k best GROUPS of a grouped memory.  Take the exhaustive row ranking of vm_topk_cosine (score_mode
 * mapping, > min_score filter, score descending, row id ascending), keep the first row of each group, return the first
 * k.  Equivalently: a group's score is the exact max over its rows, its representative the lowest row id reaching it,
 * groups ordered by (score desc, representative asc).  out_scores [Q,k] are the reference's fp64 values bit for bit,
 * out_rows [Q,k] the representatives, out_keys [Q,k] int64 (may be NULL) their group keys; -1 / 0.0 / -1 padded.
 * ALWAYS the exhaustive answer: an fp32 MFMA scan reduces scores to per-group fp32 maxima, the best k + slack groups are
 * re-scored exactly, and a query whose result cannot be proven (vm_topk_cosine's bound 2 (D + 8) 2^-24 against the
 * best rejected group's fp32 max, or more than 4096 candidate rows) is counted in *out_uncertified (may be NULL),
 * marked in out_query_flags [Q] (vm_topk_flag; may be NULL) and redone exhaustively on the device inside the same call.
 * Every row of a candidate group is re-scored, so groups of a few hundred rows or more (k = 10: an average above ~220)
 * always take that exhaustive redo: exact, but at the cost of an exhaustive search.  So does every query whose norm, or
 * a stored row's norm, is neither 0 nor in [2^-40, 2^40], the interval inside which the bound holds (vm_memory_create);
 * stored NaN / inf values are undefined, as in the reference.
 * No host read-back, no allocation: capturable.  1 <= k <= 64, Q >= 1; VM_ERR_INVALID on a memory that is not grouped.
 * Workspace: vm_topk_grouped_workspace_bytes (4 x Q x capacity bytes of per-group maxima plus a few MB). */
size_t vm_topk_grouped_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_grouped(vm_memory *mem, const void *queries, int Q, int k, int use_min_score, double min_score,
                           int score_mode, double *out_scores, int64_t *out_rows, int64_t *out_keys,
                           int32_t *out_uncertified, int32_t *out_query_flags, void *workspace, size_t workspace_bytes,
                           void *stream);
/* The same contract, exhaustive only: every row scored exactly for every query (slow; tests, and a checker). */
int vm_topk_cosine_grouped_exact(vm_memory *mem, const void *queries, int Q, int k, int use_min_score,
                                 double min_score, int score_mode, double *out_scores, int64_t *out_rows,
                                 int64_t *out_keys, void *workspace, size_t workspace_bytes, void *stream);
/* Scoped top-k: the k best rows of a tagged memory among those IN SCOPE.  scope_lo / scope_hi: device int64 [Q], one
 * inclusive tag range per query (device arrays, so that a captured graph can be replayed with another window); row r is
 * in query q's scope iff scope_lo[q] <= tag[r] <= scope_hi[q].  The result is the exhaustive row ranking of
 * vm_topk_cosine (score_mode mapping, > min_score filter, score descending, row id ascending) over the in-scope rows
 * only, first k: out_scores [Q,k] the reference's fp64 values bit for bit, out_rows [Q,k] global row ids
 * (row_id * row_stride + row_offset), -1 / 0.0 padded.  An empty scope (lo > hi, or no live row matches) gives an
 * all-padded row; with [INT64_MIN, INT64_MAX] the result equals vm_topk_cosine + vm_topk_redo_flagged.
 * ALWAYS the exhaustive answer: an fp32 MFMA scan scores the 16-row tiles that hold an in-scope row (the others cost
 * their 8-byte tags, their rows are not read), the best k + slack in-scope rows are re-scored exactly, and a query whose
 * result cannot be proven (vm_topk_cosine's bound 2 (D + 8) 2^-24 against the best in-scope fp32 score that was not
 * re-scored - out-of-scope rows never enter it -, or more than 8192 in-scope rows at the query's cut) is counted in
 * *out_uncertified (may be NULL), marked in out_query_flags [Q] (vm_topk_flag; may be NULL) and redone exhaustively over
 * its in-scope rows on the device inside the same call.  So is every query whose norm, or a stored row's norm, is
 * neither 0 nor in [2^-40, 2^40], the interval inside which the bound holds (vm_memory_create): exact, at exhaustive
 * cost; stored NaN / inf values are undefined, as in the reference.
 * No host read-back, no allocation: capturable.  1 <= k <= 64, Q >= 1; VM_ERR_INVALID on a memory that is not tagged.
 * Workspace: vm_topk_scoped_workspace_bytes (4 x Q x capacity bytes of fp32 keys plus 64 KiB x Q and a few MB). */
size_t vm_topk_scoped_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_scoped(vm_memory *mem, const void *queries, int Q, int k, const int64_t *scope_lo,
                          const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                          int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                          int32_t *out_uncertified, int32_t *out_query_flags, void *workspace, size_t workspace_bytes,
                          void *stream);
/* The same contract, exhaustive only: every in-scope pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_scoped_exact(vm_memory *mem, const void *queries, int Q, int k, const int64_t *scope_lo,
                                const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                void *workspace, size_t workspace_bytes, void *stream);
/* Row masks and masked top-k: search any set of rows.  A MASK is a device array of W = vm_memory_mask_words(mem) 32-bit
 * words (the capacity rounded up to 64 rows, / 32); several masks lie back to back, [n_masks][W].  The bit of row id r is
 * bit s & 31 of word s >> 5 with s = r mod capacity: in a linear memory s = r, in a ring the physical slot the row lives
 * in.  A bit whose slot holds no live row (past the row count, the padding, all of an empty memory) is ignored by every
 * consumer, so ~mask is meaningful and safe; masks combine with & | ~ on the caller's side.  That holds after
 * vm_memory_reset and after an erase as well, whatever the slots past the live count still hold (a reset leaves the
 * columns as they are): only the row count decides which bits count.  A mask is a statement about
 * ROW IDS: an erase renumbers rows and a ring overwrites them, after which a mask is stale exactly as a stored row id
 * is (the bit then names whichever row lives in the slot); nothing remaps it.
 * vm_topk_cosine_masked: masks [n_masks][W]; mask_index: device int32 [Q], the mask each query uses, or NULL: mask 0
 *   for every query when n_masks == 1, mask q for query q when n_masks == Q, VM_ERR_INVALID for any other n_masks.  An
 *   index outside [0, n_masks) is the EMPTY mask (an all-padded row, never an out-of-range read).  At most 2^30 words of
 *   masks per call (VM_ERR_UNSUPPORTED above).  The result is the exhaustive row ranking of vm_topk_cosine (reference
 *   fp64 cosines bit for bit, score_mode mapping, > min_score filter, score descending, row id ascending) over the
 *   selected live rows only, first k: out_scores [Q,k], out_rows [Q,k] global row ids (row_id * row_stride +
 *   row_offset), -1 / 0.0 padded.  With every bit set the result equals vm_topk_cosine + vm_topk_redo_flagged; with the
 *   mask of a tag range (vm_mask_from_scopes) it equals vm_topk_cosine_scoped.
 *   ALWAYS the exhaustive answer, like the scoped search: an fp32 MFMA scan scores the 16-row tiles in which some query
 *   selects a live row (the others cost 2 bytes of mask per query, their rows are not read), the best M = k + slack
 *   selected rows are re-scored exactly, and a query is certified when its mask selects at most M rows or the exact k-th
 *   score clears the (M+1)-th SELECTED fp32 score by vm_topk_cosine's bound 2 (D + 8) 2^-24 - unselected rows never
 *   enter it.  Any other query (VM_FLAG_GAP; VM_FLAG_OVERFLOW: more than 8192 selected rows at the query's cut) is counted
 *   in *out_uncertified (may be NULL), marked in out_query_flags [Q] (vm_topk_flag; may be NULL) and redone exhaustively
 *   over its selected rows on the device inside the same call.  The bound's norm domain is vm_topk_cosine_scoped's.
 *   Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation: capturable; a replay sees a mask
 *   rewritten in place and the rows appended since.  1 <= k <= 64, Q >= 1.
 *   Workspace: vm_topk_masked_workspace_bytes (= the scoped search's: 4 x Q x capacity bytes of keys plus 64 KiB x Q
 *   and a few MB). */
int64_t vm_memory_mask_words(const vm_memory *mem);
size_t vm_topk_masked_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_masked(vm_memory *mem, const void *queries, int Q, int k, const uint32_t *masks, int n_masks,
                          const int32_t *mask_index, int use_min_score, double min_score, int score_mode,
                          int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                          int32_t *out_uncertified, int32_t *out_query_flags, void *workspace, size_t workspace_bytes,
                          void *stream);
/* The same contract, exhaustive only: every selected pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_masked_exact(vm_memory *mem, const void *queries, int Q, int k, const uint32_t *masks, int n_masks,
                                const int32_t *mask_index, int use_min_score, double min_score, int score_mode,
                                int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                void *workspace, size_t workspace_bytes, void *stream);
/* The device-side mask builders; stream-ordered, no host read-back, capturable.  out_mask: one mask, W words.
 * vm_mask_from_rows: sets the bit of every live row named in row_ids, device int64 [n] as any search wrote them
 *   (row * row_stride + row_offset; row_stride >= 1).  -1 entries, ids not of that form and ids of rows that are not live
 *   (never appended, or overwritten by a ring) are skipped; duplicates are fine.  clear_first != 0: the mask is zeroed
 *   first; 0: the bits are ORed into what out_mask holds (atomically per word: the result does not depend on order).
 * vm_mask_from_scopes: tagged memories only (VM_ERR_INVALID otherwise).  scope_lo / scope_hi: device int64 [n_ranges],
 *   inclusive tag ranges by vm_topk_cosine_scoped's rule; a bit is set iff its slot holds a live row whose tag lies in
 *   ANY of the ranges (vm_memory_erase_scoped's selector).  Writes every word of the mask (no atomics; a slot without a
 *   live row gives 0); n_ranges == 0 gives the empty mask. */
int vm_mask_from_rows(vm_memory *mem, const int64_t *row_ids, int64_t n, int64_t row_stride, int64_t row_offset,
                      int clear_first, uint32_t *out_mask, void *stream);
int vm_mask_from_scopes(vm_memory *mem, const int64_t *scope_lo, const int64_t *scope_hi, int n_ranges,
                        uint32_t *out_mask, void *stream);
/* Span top-k: the k best rows among those whose ROW ID lies in the query's span.  Row ids are append order and append
 * order is time, so a span is "the past before this frame": what a stored frame resembles in its own past, other than a
 * moment ago (recall), or a causal limit per query.  row_lo / row_hi: device int64 [Q], both required (NULL is
 * VM_ERR_INVALID), inclusive LOCAL row ids: append order, before the row_stride / row_offset mapping.  Row r counts for
 * query q iff r is live and row_lo[q] <= r <= row_hi[q]; live means lo .. n - 1, with lo = n - capacity in a wrapped ring
 * and 0 otherwise.  Ids inside a span that are not live are ignored: ids below the oldest row, ids at or past the row
 * count, negative ids.  row_lo[q] > row_hi[q] is the EMPTY span and gives an all-padded result row; INT64_MIN .. INT64_MAX
 * is every live row.  A span is a statement about ROW IDS and goes stale after an erase, exactly as a mask does; nothing
 * remaps it.
 * The result is the exhaustive row ranking of vm_topk_cosine (reference fp64 cosines bit for bit, score_mode mapping,
 * strict > min_score filter, score descending, row id ascending) over the rows in the span only, first k: out_scores
 * [Q,k], out_rows [Q,k] global row ids (row_id * row_stride + row_offset), -1 / 0.0 padded.
 * Identities: with every span INT64_MIN .. INT64_MAX the result equals vm_topk_cosine + vm_topk_redo_flagged; on a tagged
 * memory whose tags are the row ids it equals vm_topk_cosine_scoped for the same ranges; it equals
 * vm_topk_cosine_masked with the mask of the span's rows (vm_mask_from_rows).
 * ALWAYS the exhaustive answer, like the scoped search: an fp32 MFMA scan scores the 16-row tiles that hold a wanted row -
 * whether a tile does follows from arithmetic on its row ids, so the test reads no memory and the rows of the other tiles
 * are not read -, the best M = k + max(8, k/4) in-span rows are re-scored exactly, and a query is certified when its span
 * holds at most M live rows or the exact k-th score clears the (M+1)-th IN-SPAN fp32 score by vm_topk_cosine's bound
 * 2 (D + 8) 2^-24 - rows outside the span never enter it.  Any other query (VM_FLAG_GAP; VM_FLAG_OVERFLOW: more than
 * 8192 in-span rows at the query's cut) is counted in *out_uncertified (may be NULL), marked in out_query_flags [Q]
 * (vm_topk_flag; may be NULL) and redone exhaustively over its span on the device inside the same call.  The bound's norm
 * domain is vm_topk_cosine_scoped's.
 * Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation, no synchronisation; the row count and the
 * spans are read on the device and the grids are sized from the capacity: capturable, and a replay sees spans rewritten
 * in place and the rows appended since.  1 <= k <= 64, Q >= 1; an undersized workspace is VM_ERR_NOMEM before any launch.
 * Workspace: vm_topk_span_workspace_bytes (= the scoped search's: 4 x Q x capacity bytes of keys plus 64 KiB x Q and a
 * few MB). */
size_t vm_topk_span_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_span(vm_memory *mem, const void *queries, int Q, int k, const int64_t *row_lo, const int64_t *row_hi,
                        int use_min_score, double min_score, int score_mode, int64_t row_stride, int64_t row_offset,
                        double *out_scores, int64_t *out_rows, int32_t *out_uncertified, int32_t *out_query_flags,
                        void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every in-span pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_span_exact(vm_memory *mem, const void *queries, int Q, int k, const int64_t *row_lo,
                              const int64_t *row_hi, int use_min_score, double min_score, int score_mode,
                              int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                              void *workspace, size_t workspace_bytes, void *stream);
/* Mixed-query top-k: the k best rows by a WEIGHTED SUM OF COSINES.  A mixed query c is J term vectors and J weights:
 * text plus picture in a joint space, relevance feedback (positive and negative terms), the mean over a few examples.
 * terms: [C, J, D] device vectors in the memory's dtype, 1 <= J <= 16; weights: [C, J] device fp64 (on the device, like
 * scopes and spans: a captured graph replays with rewritten weights).  masks: NULL = every live row (n_masks and
 * mask_index are then ignored); otherwise masks, n_masks and mask_index mean exactly what they mean in
 * vm_topk_cosine_masked, one mask per mixed query (mask_index [C]; NULL: n_masks == 1 or n_masks == C).
 * Score of row r for query c:  W(c, r) = sum_j w[c][j] * e_j(r),  e_j(r) = the raw reference cosine of term j and row r
 * (vm_topk_cosine's fp64 value; 0.0 when either norm is zero), the sum started at 0.0 and taken j = 0 .. J-1 left to
 * right, one rounding per product and one per addition, never fused.  So J = 1, w = 1.0 gives the reference cosine bit
 * for bit (the result equals vm_topk_cosine / vm_topk_cosine_masked), and appended terms of weight 0.0 change no bit.
 * Result: the live rows the mask selects ranked by (W descending, row id ascending), those with W > min_score kept when
 * use_min_score != 0 (strict; the scores are raw only: the unit-interval mapping has no meaning outside [-1, 1]), first k:
 * out_scores [C,k] the fp64 W bit for bit, out_rows [C,k] global row ids (row_id * row_stride + row_offset), 0.0 / -1
 * padded.  The result of a query depends on the memory, its own terms, weights and mask and the arguments only, not on
 * the other queries of the call.  Non-finite weights are undefined, as stored NaN is.
 * ALWAYS the exhaustive answer: the fp32 MFMA tile scan scores the J terms as the 16 columns of one query tile and sums
 * them, scaled by fl32(w_j / ||term_j||), into ONE fp32 score B per (query, row); the best M = k + max(8, k/4) selected
 * rows are re-scored exactly, and a query is certified when its mask selects at most M rows or the exact k-th W clears
 * the (M+1)-th scanned score by eps_mix = A (2 (D + 8) 2^-24 + 2^-21), A = sum_j |w_j|, strictly.  The bound holds when
 * every nonzero |w_j| lies in [2^-20, 2^20] and every term and stored norm is 0 or in [2^-40, 2^40]; outside, and for any
 * other query (VM_FLAG_GAP; VM_FLAG_OVERFLOW: more than 8192 selected rows at the query's cut), the query is counted in
 * *out_uncertified (may be NULL), marked in out_query_flags [C] (vm_topk_flag; may be NULL) and redone exhaustively over
 * its selected rows on the device inside the same call.
 * Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation, no synchronisation: capturable; a replay
 * sees weights, terms and masks rewritten in place and the rows appended since.  1 <= k <= 64, C >= 1.  VM_ERR_INVALID
 * (with a vm_last_error text) for J outside [1, 16], k outside [1, 64], NULL terms, weights or outputs, a workspace
 * below vm_topk_mix_workspace_bytes, masks that are not 4-byte aligned or whose count fits no rule above; the workspace
 * must be 256-byte, terms 16-byte and weights 8-byte aligned.
 * Workspace: vm_topk_mix_workspace_bytes (4 x C x capacity bytes of keys, 32 x D bytes of packed terms per query, plus
 * 64 KiB x C and a few MB). */
size_t vm_topk_mix_workspace_bytes(const vm_memory *mem, int C, int k);
int vm_topk_cosine_mix(vm_memory *mem, const void *terms, const double *weights, int C, int J, int k,
                       const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                       double min_score, int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                       int32_t *out_uncertified, int32_t *out_query_flags, void *workspace, size_t workspace_bytes,
                       void *stream);
/* The same contract, exhaustive only: every selected (query, row) pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_mix_exact(vm_memory *mem, const void *terms, const double *weights, int C, int J, int k,
                             const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                             double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                             int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream);
/* Any/all top-k: the k best rows by the MAXIMUM or the MINIMUM OF WEIGHTED COSINES over the terms of a fold query.
 * VM_FOLD_MAX ("any", OR): rows that resemble any frame of a chunk / any of a few questions - the score by which the
 * reference links a new batch to stored chunks (the maximum per stored id over the batch's result lists).  VM_FOLD_MIN
 * ("all", AND): rows whose WORST term is best - text and example picture at once; a weighted sum cannot say that, one
 * strong term carries a row.
 * terms, weights, C, J, masks, n_masks, mask_index, the min-score pair, row_stride / row_offset, the outputs, the flags, the
 * workspace and the stream mean exactly what they mean in vm_topk_cosine_mix; one mask per fold query.
 * Score of row r for query c, with p_j = w[c][j] * e_j(r) (one fp64 rounding) and e_j(r) the raw reference cosine of term j
 * and row r (vm_topk_cosine's fp64 value; 0.0 when either norm is zero):
 *     acc = p_0, arg = 0;  for j = 1 .. J-1:  if p_j > acc (max) / p_j < acc (min):  acc = p_j, arg = j
 *     F(c, r) = acc,  T(c, r) = arg
 * The compare is strict: the first term wins a tie, and +0.0 is never replaced by -0.0 (nor -0.0 by +0.0).  The padding
 * columns J .. 15 of the query tile never take part.  A ZERO WEIGHT IS NOT NEUTRAL here, unlike in vm_topk_cosine_mix: its
 * product +-0.0 takes part in the maximum / minimum like any other value.  So J = 1, w = 1.0 gives the reference cosine
 * bit for bit (the result equals vm_topk_cosine / vm_topk_cosine_masked), permuting the terms with their weights changes no
 * row and no score bit (only T) - with ONE exception: where a row's products tie as zeros of both signs (a zero weight, or a
 * cosine that is exactly 0.0), the first of them in term order gives F its sign, so a permutation can turn a +0.0 score into
 * -0.0 or back; the value, the ranking and every nonzero score are unaffected - and appending a copy of a term with its
 * weight changes nothing at all.
 * Result: the live rows the mask selects ranked by (F DESCENDING, row id ascending) for BOTH ops, those with F > min_score
 * kept when use_min_score != 0 (strict, on the raw value), first k: out_scores [C,k] the fp64 F bit for bit, out_rows [C,k]
 * global row ids (row_id * row_stride + row_offset), 0.0 / -1 padded; out_terms: int32 [C,k] or NULL, T of each returned row
 * (which frame of the chunk linked, which question matched), -1 where the row is -1.  The result of a query depends on the
 * memory, its own terms, weights and mask and the arguments only, not on the other queries of the call.  Non-finite weights
 * are undefined, as stored NaN is.
 * ALWAYS the exhaustive answer: the fp32 MFMA tile scan scores the J terms as the 16 columns of one query tile, scales
 * column j by fl32(w_j / ||term_j||) and takes the maximum / minimum over the J columns into ONE fp32 score B per (query,
 * row); the best M = k + max(8, k/4) selected rows are re-scored exactly, and a query is certified when its mask selects at
 * most M rows or the exact k-th F clears the (M+1)-th scanned score by eps_fold = A (2 (D + 8) 2^-24 + 2^-21),
 * A = max_j |w_j|, strictly (max and min move by no more than their most-moved argument).  The bound holds when every
 * nonzero |w_j| lies in [2^-20, 2^20] and every term and stored norm is 0 or in [2^-40, 2^40]; outside, and for any other
 * query (VM_FLAG_GAP; VM_FLAG_OVERFLOW: more than 8192 selected rows at the query's cut), the query is counted in
 * *out_uncertified (may be NULL), marked in out_query_flags [C] (vm_topk_flag; may be NULL) and redone exhaustively over its
 * selected rows on the device inside the same call.
 * Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation, no synchronisation: every launch reads the
 * row count on the device and sizes its grid from the capacity, so the call is capturable; a replay sees weights, terms and
 * masks rewritten in place and the rows appended since.  1 <= k <= 64, 1 <= C <= 2^20.  VM_ERR_INVALID (with a vm_last_error
 * text) for an op that is no vm_fold_op and for everything vm_topk_cosine_mix refuses, before any launch, with the outputs
 * untouched; the workspace must be 256-byte, terms 16-byte and weights 8-byte aligned.
 * Workspace: vm_topk_fold_workspace_bytes (= the mixed search's); 0 for arguments out of range. */
enum vm_fold_op { VM_FOLD_MAX = 0, VM_FOLD_MIN = 1 };
size_t vm_topk_fold_workspace_bytes(const vm_memory *mem, int C, int k);
int vm_topk_cosine_fold(vm_memory *mem, const void *terms, const double *weights, int C, int J, int k, int op,
                        const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                        double min_score, int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                        int32_t *out_terms, int32_t *out_uncertified, int32_t *out_query_flags, void *workspace,
                        size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every selected (query, row) pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_fold_exact(vm_memory *mem, const void *terms, const double *weights, int C, int J, int k, int op,
                              const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                              double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                              int64_t *out_rows, int32_t *out_terms, void *workspace, size_t workspace_bytes,
                              void *stream);
/* Biased top-k: the k best rows by COSINE PLUS A PER-ROW PRIOR.  A preference that is not a filter: recency, a decaying
 * or reinforced strength per stored frame, an importance weight from metadata, a boost for the rows another retrieval leg
 * found.  The best k rows of cos + prior do not follow from the best k rows of cos, however large a pool is fetched.
 * The bias column: a device array of S = vm_memory_bias_stride(mem) fp32 values, S = 32 x vm_memory_mask_words (the
 * capacity rounded up to 64); several columns lie back to back as [n_bias][S], 16-byte aligned.  Entry s belongs to the
 * row in physical slot s = row_id mod capacity - the masks' rule exactly -, an entry whose slot holds no live row is ignored
 * by every consumer, and a column speaks about ROW IDS: it goes stale after an erase or a ring overwrite, as a mask does.
 * bias_index: device int32 [Q] or NULL.  NULL: column 0 serves every query when n_bias == 1, column q serves query q when
 * n_bias == Q; any other count with a NULL index is VM_ERR_INVALID.  An index outside [0, n_bias) is the ZERO column, never
 * an out-of-range read.  bias_weight: device fp64 [Q] (beta_q; on the device, like the mixed weights: a captured graph
 * replays with rewritten weights), or NULL for 1.0 for every query.  More than 2^30 bias values in one call are
 * VM_ERR_UNSUPPORTED (the mask limit's answer), so that offsets stay 32-bit.
 * Score of row r for query q:  S(q, r) = e(q, r) + beta_q * b[slot(r)],  e = the raw reference cosine (vm_topk_cosine's
 * fp64 value; 0.0 when either norm is zero), b widened exactly to fp64, one fp64 rounding for the product and one for the
 * sum, never fused.  masks: NULL = every live row (n_masks and mask_index are then ignored); otherwise masks, n_masks and
 * mask_index mean exactly what they mean in vm_topk_cosine_masked.
 * Result: the live rows the mask selects ranked by (S descending, row id ascending), those with S > min_score kept when
 * use_min_score != 0 (strict; raw only: S is not confined to [-1, 1], so there is no score_mode), first k: out_scores [Q,k]
 * the fp64 S bit for bit, out_rows [Q,k] global row ids (row_id * row_stride + row_offset), 0.0 / -1 padded.  The result of a
 * query depends on the memory, its own vector, column, weight and mask and the arguments only, not on the other queries of
 * the call.  Non-finite bias values or weights are undefined, as stored NaN is.
 * Identities: beta_q = 0, or a column of zeros, gives vm_topk_cosine + vm_topk_redo_flagged bit for bit, and with a mask
 * vm_topk_cosine_masked: the reference cosine is never -0.0 (its dot product starts at +0.0, a zero norm gives 0.0), and
 * e + (+-0.0) = e for every other e.
 * ALWAYS the exhaustive answer, like the masked search: the fp32 MFMA tile scan computes, one query per column,
 * B = fl32(fl32(fl32(1 / ||q||) * s) + fl32(fl32(beta) * b)) per selected live row from its fp32 score s and one 4-byte bias
 * value read next to the row; the best M = k + max(8, k/4) selected rows by B are re-scored exactly, and a query is certified
 * when its mask selects at most M live rows or the exact k-th S is strictly above B* + eps_bias(D, B*), B* the (M+1)-th
 * scanned score and eps_bias(D, B) = 2 (D + 8) 2^-24 + 2^-21 + 2^-22 |B|.  The bound holds when |beta| is 0 or lies in
 * [2^-20, 2^20], every selected row's |b| <= 2^40 and the query's and every stored norm is 0 or in [2^-40, 2^40]; outside,
 * and for any other query (VM_FLAG_GAP; VM_FLAG_OVERFLOW: more than 8192 selected rows at the query's cut), the query is
 * counted in *out_uncertified (may be NULL), marked in out_query_flags [Q] (vm_topk_flag; may be NULL) and redone
 * exhaustively over its selected rows on the device inside the same call.
 * Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation, no synchronisation: every launch reads the
 * row count on the device and sizes its grid from the capacity, so the call is capturable; a replay sees bias values,
 * weights, indices, queries and masks rewritten in place and the rows appended since.  1 <= k <= 64, Q >= 1.
 * VM_ERR_INVALID (with a vm_last_error text) for k outside [1, 64], Q < 1, NULL queries, bias or outputs, row_stride < 1,
 * a bias that is not 16-byte aligned or whose count fits no rule above, the mask operand's refusals of
 * vm_topk_cosine_mix, a workspace below vm_topk_bias_workspace_bytes; the workspace must be 256-byte, queries 16-byte and
 * bias_weight 8-byte aligned.  All before any launch, with the outputs untouched.
 * Workspace: vm_topk_bias_workspace_bytes (the masked search's plus five small per-query arrays); 0 for arguments out of
 * range. */
int64_t vm_memory_bias_stride(const vm_memory *mem);
size_t vm_topk_bias_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_biased(vm_memory *mem, const void *queries, int Q, int k, const float *bias, int n_bias,
                          const int32_t *bias_index, const double *bias_weight, const uint32_t *masks, int n_masks,
                          const int32_t *mask_index, int use_min_score, double min_score, int64_t row_stride,
                          int64_t row_offset, double *out_scores, int64_t *out_rows, int32_t *out_uncertified,
                          int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every selected (query, row) pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_biased_exact(vm_memory *mem, const void *queries, int Q, int k, const float *bias, int n_bias,
                                const int32_t *bias_index, const double *bias_weight, const uint32_t *masks,
                                int n_masks, const int32_t *mask_index, int use_min_score, double min_score,
                                int64_t row_stride, int64_t row_offset, double *out_scores, int64_t *out_rows,
                                void *workspace, size_t workspace_bytes, void *stream);
/* The device-side bias builders; stream-ordered, no host read-back, capturable.  out_bias: ONE column, S fp32 values,
 * 16-byte aligned.
 * vm_bias_from_rows: stores values[i] (device fp32 [n]) in the slot of every live row named in row_ids, device int64 [n] as
 *   any search wrote them (row * row_stride + row_offset; row_stride >= 1).  -1 entries, ids not of that form and ids of
 *   rows that are not live are skipped: vm_mask_from_rows's rules.  clear_first != 0: the column is zeroed first; 0: the
 *   other entries keep what they hold.  Duplicates that carry DIFFERENT values leave one of them, which one is not
 *   defined (plain stores race); duplicates with one value are fine.
 * vm_bias_from_tags: tagged memories only (VM_ERR_INVALID otherwise).  Linear recency: a live slot with tag t != INT64_MIN
 *   gets b = (float)(per_ms * (double)d), d = (t & (2^40 - 1)) - t_ref_ms exact in int64 and in fp64, one fp64 rounding for
 *   the product, then round to nearest even to fp32.  Untagged live rows and slots without a live row get `fill`.  Writes
 *   all S entries.  per_ms = 1e-6: a frame loses 0.06 of score per minute of age; any other shape of decay is the
 *   caller's own expression over the column. */
int vm_bias_from_rows(vm_memory *mem, const int64_t *row_ids, const float *values, int64_t n, int64_t row_stride,
                      int64_t row_offset, int clear_first, float *out_bias, void *stream);
int vm_bias_from_tags(vm_memory *mem, int64_t t_ref_ms, double per_ms, float fill, float *out_bias, void *stream);
/* Diverse top-k: maximal marginal relevance (MMR).  The k answers of a query are picked one after another from a POOL of
 * its best rows, and each pick pays for its resemblance to the rows picked before it, so that near-identical frames - a
 * static camera, a replayed scene, one shot in two uploads - do not fill the k places.
 * queries: [Q, D] in the memory's dtype; 1 <= k <= pool <= 64; lam: device fp64 [Q] (on the device, like weights, scopes
 * and spans: a captured graph replays with rewritten values).  masks: NULL = every live row (n_masks and mask_index are
 * then ignored); otherwise masks, n_masks and mask_index mean exactly what they mean in vm_topk_cosine_masked.
 * The pool of query q: the exhaustive ranking of vm_topk_cosine over the live rows the mask selects, those with
 * e > min_score kept when use_min_score != 0 (strict, on the raw cosine; there is no score mode), first `pool` entries:
 * rows r_0 .. r_{np-1}, np <= pool, e_i the raw reference cosine bit for bit, ordered (e descending, row id ascending).
 * The greedy pick, in fp64 with one rounding per operation, never fused:  mu = 1.0 - lam;  sim(i, j) = the reference
 * cosine BETWEEN stored rows r_i and r_j (the dot of vm_topk_cosine's arithmetic over the two rows, divided by the product
 * of their stored fp64 norms; 0.0 when either norm is 0), which is symmetric bit for bit.  Step 0 takes r_0, with
 * red = 0.0.  At step t >= 1 every unpicked i has red_i = the maximum (plain >, from 0.0) of sim(i, s) over the picked s
 * and the value  v_i = (lam * e_i) - (mu * red_i);  the largest v_i wins, ties - -0.0 against +0.0 included - go to the
 * smaller row id.  min(k, np) picks are made.
 * Outputs, in pick order: out_rows [Q,k] global row ids (row_id * row_stride + row_offset), out_scores [Q,k] the
 * relevance e of each pick, out_mmr [Q,k] the v at which it was picked (step 0: (lam * e_0) - (mu * 0.0)); -1 / 0.0 / 0.0
 * padded.  Consequences: lam = 1.0 gives the rows and scores of vm_topk_cosine (or _masked), first k, bit for bit,
 * whatever the pool; pool == k only reorders the top k; the result of a query depends on the memory, its own query, lam
 * and mask and the arguments only, not on the other queries of the call.  A finite lam outside [0, 1] is still defined by
 * the formula; a non-finite lam is undefined, as stored NaN is.
 * The pool stage IS vm_topk_cosine_masked (or, without masks, vm_topk_cosine_span with the open span) with k = pool:
 * always the exhaustive answer, its uncertified queries counted in *out_uncertified (may be NULL), marked in
 * out_query_flags [Q] (vm_topk_flag; may be NULL) and redone inside the call.  Then one kernel scores the pool's pairs
 * and one wave per query picks.  Any memory: plain, grouped, tagged, ring.  No host read-back, no allocation, no
 * synchronisation: capturable; a replay sees lam, queries and masks rewritten in place and the rows appended since.
 * VM_ERR_INVALID (with a vm_last_error text) for k or pool outside [1, 64], k > pool, Q < 1, NULL queries, lam or
 * outputs (all three are required), row_stride < 1, masks that are not 4-byte aligned or whose count fits no rule of the
 * masked search, misaligned workspace (256 bytes), queries (16) or lam (8); VM_ERR_NOMEM for a workspace below
 * vm_topk_diverse_workspace_bytes; VM_ERR_UNSUPPORTED above 2^30 words of masks or D > 5,120.  All before any launch,
 * with the outputs untouched.
 * Workspace: vm_topk_diverse_workspace_bytes(mem, Q, pool) (the masked search's for k = pool, plus 32 KiB x Q of pair
 * cosines and the pool); 0 for arguments out of range. */
size_t vm_topk_diverse_workspace_bytes(const vm_memory *mem, int Q, int pool);
int vm_topk_cosine_diverse(vm_memory *mem, const void *queries, int Q, int k, int pool, const double *lam,
                           const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                           double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                           int64_t *out_rows, double *out_mmr, int32_t *out_uncertified, int32_t *out_query_flags,
                           void *workspace, size_t workspace_bytes, void *stream);
/* The same contract with the exhaustive-only pool: every selected pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_diverse_exact(vm_memory *mem, const void *queries, int Q, int k, int pool, const double *lam,
                                 const uint32_t *masks, int n_masks, const int32_t *mask_index, int use_min_score,
                                 double min_score, int64_t row_stride, int64_t row_offset, double *out_scores,
                                 int64_t *out_rows, double *out_mmr, void *workspace, size_t workspace_bytes,
                                 void *stream);
/* Scoped grouped top-k: the k best GROUPS of a tagged AND grouped memory among the rows IN SCOPE - "the k best scenes of
 * video 7 between minute 10 and minute 20".  scope_lo / scope_hi: device int64 [Q], both required, inclusive tag ranges
 * by vm_topk_cosine_scoped's rule (row r is in query q's scope iff scope_lo[q] <= tag[r] <= scope_hi[q]).
 * Groups are what they are everywhere else: maximal runs of equal group ordinals over ALL live rows.  A scope does not
 * redefine them: an out-of-scope row between two in-scope rows of one group does not split the group, and removing rows
 * from view never merges two groups.
 * Result for query q: take the exhaustive row ranking of vm_topk_cosine_scoped (in-scope live rows only, the raw
 * reference cosine mapped by score_mode, the strict > min_score filter, raw score descending, row id ascending), keep the
 * first row of each group, return the first k.  Equivalently: a group's score is the exact max over its IN-SCOPE rows,
 * its representative the lowest in-scope row id reaching that max; a group with no in-scope row does not exist for this
 * query.  out_scores [Q,k] are the reference's fp64 values bit for bit, out_rows [Q,k] row ids (no stride or offset, as
 * in vm_topk_cosine_grouped), out_keys [Q,k] int64 (may be NULL) the representatives' group keys; 0.0 / -1 / -1 padded.
 * Identities: with every scope [INT64_MIN, INT64_MAX] the three outputs equal vm_topk_cosine_grouped's; on a memory
 * where every row is its own group, scores and rows equal vm_topk_cosine_scoped's with row_stride 1 and row_offset 0.
 * ALWAYS the exhaustive answer, as with both parents: an fp32 MFMA scan of the 16-row tiles that hold an in-scope row
 * reduces the in-scope scores to per-group fp32 maxima, the in-scope rows of the best k + slack groups are re-scored
 * exactly, and a query whose result cannot be proven (vm_topk_cosine's bound 2 (D + 8) 2^-24 against the fp32 max over
 * the in-scope rows of the best group that was not re-scored, or candidate groups of more than 4096 rows together - all
 * their rows count, in scope or not) is counted in *out_uncertified (may be NULL), marked in out_query_flags [Q]
 * (vm_topk_flag; may be NULL) and redone exhaustively over its in-scope rows on the device inside the same call.  So is
 * every query whose norm, or a stored row's norm, is neither 0 nor in [2^-40, 2^40] (vm_memory_create).
 * No host read-back, no allocation, no synchronisation; the row count and the scopes are read on the device and the
 * grids are sized from the capacity: capturable, and a replay after an append or with rewritten scopes sees the new
 * state.  1 <= k <= 64, Q >= 1; VM_ERR_INVALID on a memory that is not both tagged and grouped
 * (vm_memory_create_tagged with grouped != 0), on a NULL scope array and on k outside its range; VM_ERR_NOMEM on an
 * undersized workspace, before any launch.
 * Workspace: vm_topk_grouped_scoped_workspace_bytes (4 x Q x capacity bytes of per-group maxima plus a few MB). */
size_t vm_topk_grouped_scoped_workspace_bytes(const vm_memory *mem, int Q, int k);
int vm_topk_cosine_grouped_scoped(vm_memory *mem, const void *queries, int Q, int k, const int64_t *scope_lo,
                                  const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                  double *out_scores, int64_t *out_rows, int64_t *out_keys, int32_t *out_uncertified,
                                  int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every in-scope pair scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_grouped_scoped_exact(vm_memory *mem, const void *queries, int Q, int k, const int64_t *scope_lo,
                                        const int64_t *scope_hi, int use_min_score, double min_score, int score_mode,
                                        double *out_scores, int64_t *out_rows, int64_t *out_keys, void *workspace,
                                        size_t workspace_bytes, void *stream);
/* Clip search: where does a SEQUENCE of frames occur in the memory - "have I seen these 16 frames before, and where?".
 * The memory stores one row per frame in time order; the aligned counterpart of the reference's chunk-to-chunk link
 * (src/components/pre_llm_injector.py:346-372, one vector per chunk) is a score per START ROW.
 * clips [C, L, D] dtype, 1 <= L <= 16, C >= 1, 1 <= k <= 64, 1 <= min_sep <= 32 (VM_ERR_INVALID outside); any memory
 * (plain, grouped, tagged, ring).
 * Window: for a live start row r, window r is the rows r .. r+L-1 (live ids lo .. n-1 as in vm_memory_events).  It is
 *   VALID iff all L rows are live and, on a tagged memory, no row r+1 .. r+L-1 has a TAG BREAK against its predecessor -
 *   the tag part of vm_memory_events' opening rule: exactly one of the two tags is INT64_MIN; or neither is and the
 *   sources differ; or neither is, max_gap_ms >= 0 and the clock step is negative or above max_gap_ms.  A window never
 *   spans two videos.  max_gap_ms >= 0 on an untagged memory: VM_ERR_INVALID.
 * Scope: scope_lo / scope_hi device int64 [C], or both NULL.  A window is IN SCOPE iff every one of its L rows is, by
 *   vm_topk_cosine_scoped's rule.  Scopes on an untagged memory, or one NULL and one not: VM_ERR_INVALID.
 * Score: W(r) = (e_0 + e_1 + ... + e_{L-1}) / L, e_i the raw reference cosine of clip frame i and row r+i (fp64 on the
 *   stored 16-bit values, the stored norm, the zero-norm guard, as vm_topk_cosine); the sum starts from 0.0 and runs left
 *   to right with one rounding per addition, then one correctly rounded division by (double)L.  L = 1 makes W the reference
 *   cosine bit for bit.  The shown score is the score_mode mapping of W; the filter is strict > min_score on it.
 * Peaks: a COMPETITOR of r is a valid, in-scope window r' != r with |r' - r| < min_sep; r is a PEAK iff it ranks before
 *   every competitor in (raw W descending, start row ascending).  Two peaks are therefore at least min_sep rows apart;
 *   min_sep = 1 makes every valid in-scope window a peak.  This is LOCAL-MAXIMUM suppression, not greedy suppression: in a
 *   chain A > B > C whose neighbours are closer than min_sep only A is a peak (greedy would keep C as well).
 * Result per clip: the peaks ranked by (raw W descending, start ascending), filtered, first k.  out_scores [C,k] the shown
 *   fp64 values bit for bit, out_rows [C,k] the START row ids (no stride or offset: a row-sharded memory has no consecutive
 *   rows); 0.0 / -1 padded.  It depends on the memory, the clip and its own arguments only: not on C, the other clips, the
 *   launch geometry or the workspace size.
 * ALWAYS the exhaustive answer: an fp32 MFMA scan scores every live row against the 16 C frames, each window's fp32 mean
 *   lies within eps_w = 2 (D + 8) 2^-24 + 2^-23 of W, windows that a competitor exceeds by more than 2 eps_w are dropped
 *   as provably no peaks, the best k + slack of the rest are re-scored exactly with their competitors, and a clip whose
 *   result cannot be proven is counted in *out_uncertified (may be NULL; accumulates), marked in out_query_flags [C]
 *   (vm_topk_flag; may be NULL) and redone exhaustively on the device inside the same call.  So is every clip with a frame
 *   norm, or a stored row's norm, neither 0 nor in [2^-40, 2^40] (vm_memory_create).
 * No allocation, no synchronisation, no host read-back; the row count and the scopes are read on the device and the grids
 * are sized from the capacity: capturable.  An undersized workspace is refused with VM_ERR_NOMEM before any launch; a NaN
 * min_score with use_min_score is VM_ERR_INVALID.
 * Workspace: vm_topk_clip_workspace_bytes = 64 x C x capacity bytes of fp32 scores (16 columns per clip) + 16 x C x
 *   capacity of window scores, keys and exact redo scores + 64 KiB x C and a few MB. */
size_t vm_topk_clip_workspace_bytes(const vm_memory *mem, int C, int L, int k);
int vm_topk_cosine_clip(vm_memory *mem, const void *clips, int C, int L, int k, int min_sep, int64_t max_gap_ms,
                        const int64_t *scope_lo, const int64_t *scope_hi, int use_min_score, double min_score,
                        int score_mode, double *out_scores, int64_t *out_rows, int32_t *out_uncertified,
                        int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every valid in-scope window scored exactly (slow; tests, and a checker). */
int vm_topk_cosine_clip_exact(vm_memory *mem, const void *clips, int C, int L, int k, int min_sep, int64_t max_gap_ms,
                              const int64_t *scope_lo, const int64_t *scope_hi, int use_min_score, double min_score,
                              int score_mode, double *out_scores, int64_t *out_rows, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Sequence search: where do J ORDERED steps occur in the memory, each at most max_step rows after the one before -
 * "someone opens the door, THEN sits down, THEN picks up the phone".  The clip search scores step i against row r + i
 * exactly; here the steps may be text embeddings (no frame rate), the scene may play faster or slower, and the novelty gate
 * may have thinned the rows: the alignment is a dynamic programme over the rows, and a hit is reported by its END row.
 * steps [C, J, D] dtype, 1 <= J <= 16, 1 <= max_step = G <= 16, 1 <= k <= 64, 1 <= min_sep <= 32, C >= 1 (VM_ERR_INVALID
 * outside); any memory (plain, grouped, tagged, ring).  max_gap_ms as in vm_topk_cosine_clip; >= 0 on an untagged memory:
 * VM_ERR_INVALID.  masks / n_masks / mask_index: exactly vm_topk_cosine_masked's operand, one mask per sequence; masks NULL
 * = every live row (n_masks and mask_index are then ignored).
 * Eligibility: row r is ELIGIBLE for sequence c iff it is live and c's mask selects it.
 * Step score: e_j(r) = the raw reference cosine of step j and row r, vm_topk_cosine's fp64 value, 0.0 when either norm is 0.
 * Chains: rows r_0 < r_1 < ... < r_{J-1}, every r_j eligible, 1 <= r_j - r_{j-1} <= G and, on a tagged memory, no row in
 *   r_{j-1}+1 .. r_j with a TAG BREAK against its predecessor (vm_topk_cosine_clip's rule, max_gap_ms between ADJACENT rows
 *   included).  A chain never spans two videos; it may step over rows that the mask does not select.
 * Score, in fp64, one rounding per operation, never fused:
 *   P_0(r) = 0.0 + e_0(r) for eligible r;
 *   for j >= 1 and eligible r: among the d in 1 .. G for which P_{j-1}(r - d) exists and the tag rule allows the step, the
 *   largest P_{j-1}(r - d), ties to the SMALLEST d; pred_j(r) = r - d; P_j(r) = that value + e_j(r).  P_j(r) does not exist
 *   when r is not eligible or no such d exists;
 *   A(r) = P_{J-1}(r) / (double)J; r is an END iff A(r) exists.
 *   Rounding is monotone, so A(r) is the maximum over all chains ending at r of the left-to-right rounded sum of the chain's
 *   step scores, divided by J; and A(r) does not decrease when G grows (the chains of G are chains of G + 1).
 * Peaks: a COMPETITOR of r is an END r' != r with |r' - r| < min_sep; r is a PEAK iff it ranks before every competitor in
 *   (raw A descending, end row ascending): local-maximum suppression, not greedy, as in the clip search.
 * Result per sequence: the peaks in that order, the score_mode mapping, the strict > min_score filter on the shown score,
 *   first k.  out_scores [C,k] the shown fp64 value bit for bit; out_rows [C,k] the END row ids (no stride or offset);
 *   out_step_rows [C,k,J] int64 (may be NULL) the chain r_0 .. r_{J-1} obtained by following pred back from the end;
 *   out_step_scores [C,k,J] fp64 (may be NULL) e_j(r_j) bit for bit.  Padding 0.0 / -1 / -1 / 0.0.  The result depends on the
 *   memory, the sequence, its mask and its own arguments only.
 * Identities: J = 1, min_sep = 1 is vm_topk_cosine (with a mask: vm_topk_cosine_masked); G = 1 without a mask is
 *   vm_topk_cosine_clip with L = J and the same min_sep, max_gap_ms, score mode and filter, out_rows = its rows + J - 1;
 *   G = 1 with the mask of a scope (vm_mask_from_scopes) is the clip search with that scope.
 * ALWAYS the exhaustive answer: the clip search's fp32 scan of the 16 C steps, the J layers in fp64 over those scores per
 *   segment of end rows (each layer moves no more than its most-moved argument: the fp32 image of A lies within eps_seq =
 *   2 (D + 8) 2^-24 + 2^-23 of A), the clip search's possible-peak filter and selection, the exact layers on the cone of each
 *   of the best k + slack candidates, and a sequence whose result cannot be proven is counted in *out_uncertified (may be
 *   NULL; accumulates), marked in out_query_flags [C] (vm_topk_flag; may be NULL) and redone exhaustively on the device
 *   inside the same call - exact layers over all rows -, as is every sequence with a step norm, or a stored row's norm,
 *   neither 0 nor in [2^-40, 2^40].  Every live row is scanned: a mask does not skip tiles.
 * No allocation, no synchronisation, no host read-back; the row count, the steps and the masks are read on the device and
 * the grids are sized from the capacity: capturable.  Errors are reported before any launch, the outputs untouched:
 * VM_ERR_INVALID for a count out of range, NULL steps / out_scores / out_rows, a NaN min_score with use_min_score, a mask
 * operand vm_topk_cosine_mix refuses, a workspace not 256-byte or steps not 16-byte aligned; VM_ERR_NOMEM for a workspace
 * below vm_topk_seq_workspace_bytes (0 for arguments out of range); VM_ERR_UNSUPPORTED above 2^30 words of masks.
 * Workspace: 64 x C x capacity bytes of fp32 scores + 24 x C x capacity of end scores, keys and the two exact layers of
 *   the redo + 64 KiB x C and a few MB. */
size_t vm_topk_seq_workspace_bytes(const vm_memory *mem, int C, int J, int k);
int vm_topk_cosine_seq(vm_memory *mem, const void *steps, int C, int J, int k, int max_step, int min_sep,
                       int64_t max_gap_ms, const uint32_t *masks, int n_masks, const int32_t *mask_index,
                       int use_min_score, double min_score, int score_mode, double *out_scores, int64_t *out_rows,
                       int64_t *out_step_rows, double *out_step_scores, int32_t *out_uncertified,
                       int32_t *out_query_flags, void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: the exact layers over all rows for every sequence (slow; tests, and a checker). */
int vm_topk_cosine_seq_exact(vm_memory *mem, const void *steps, int C, int J, int k, int max_step, int min_sep,
                             int64_t max_gap_ms, const uint32_t *masks, int n_masks, const int32_t *mask_index,
                             int use_min_score, double min_score, int score_mode, double *out_scores, int64_t *out_rows,
                             int64_t *out_step_rows, double *out_step_scores, void *workspace, size_t workspace_bytes,
                             void *stream);
/* Range search: EVERY row above a threshold, in time order - "which frames of this video show X?" has no k.  The
 * threshold is the reference's own notion of relevance (`vector.similarity.cosine(...) > 0.3`,
 * src/pipeline/retriever_hybrid.py:296-298; `>= compression_threshold`, :494-504); this call returns all of what passes
 * it, not the best 64.
 * Hit rule: for query q a hit is a live row r that is in q's scope when scopes are given (scope_lo[q] <= tag[r] <=
 *   scope_hi[q], vm_topk_cosine_scoped's rule) and whose shown score - the reference cosine of vm_topk_cosine, fp64 on the
 *   stored 16-bit values, zero-norm guard, then the score_mode mapping - is STRICTLY above min_score, like use_min_score.
 *   A zero row or a zero query scores 0.0 and is a hit iff the shown score of 0.0 is above min_score.
 * Result: the hits in ASCENDING ROW ID: append order, oldest first in a ring, time order within a video.  The first
 *   max_hits are written, out_rows [Q, max_hits] = row_id * row_stride + row_offset and out_scores [Q, max_hits] the
 *   reference's fp64 values bit for bit; the rest is padded with -1 / 0.0.  out_counts[q] (device int64 [Q]) is the TOTAL
 *   number of hits, also when it exceeds max_hits: the caller sees the truncation.  max_hits = 0 is a count-only call
 *   (out_rows / out_scores may then be NULL).  The result depends on the memory, the query, its scope and the threshold
 *   only: not on Q, the other queries of the call, the launch geometry or the workspace size.
 * Scopes: scope_lo / scope_hi device int64 [Q], or both NULL = every live row, on any memory (plain, grouped, tagged,
 *   ring).  Non-NULL scopes on an untagged memory, or one NULL and one not: VM_ERR_INVALID.  An empty scope (lo > hi, or
 *   no live row matches) gives count 0.
 * Thresholds: NaN is VM_ERR_INVALID; -inf, or anything below every score, returns every in-scope row; >= 2 returns none.
 * ALWAYS the exhaustive answer, and there are no flags: the cut is known before the scan starts.  An fp32 MFMA scan bounds
 *   each pair's exact cosine from above by (double)fp32_score / ||q|| + 2 (D + 8) 2^-24 (vm_topk_cosine's bound); a pair
 *   whose bound's shown score is not above min_score is provably no hit and is dropped unscored, every other pair is
 *   re-scored exactly and is a hit iff its exact shown score passes.  out_rescored[q] (device int64 [Q], may be NULL):
 *   the pairs of query q that were scored exactly in this call (>= out_counts[q]; equal when no score lies within the
 *   bound of the threshold).  Order comes from prefix sums over separate launches: deterministic, no atomics.
 *   The bound holds while the query's norm and every stored row's norm are 0 or lie in [2^-40, 2^40] (vm_memory_create);
 *   outside that interval every in-scope pair of the query is re-scored exactly (out_rescored[q] = its in-scope rows):
 *   exact, at exhaustive cost.  Stored NaN / inf values are undefined, as in the reference.
 * No allocation, no synchronisation, no host read-back; the row count is read on the device and launches are sized from
 * the capacity: capturable, and a replay after an append sees the new rows.  Calls are stream-ordered per handle.
 * Workspace: vm_range_workspace_bytes(mem, Q) = with P = capacity rounded up to 64 rows and C = ceil(P / 4096) chunks,
 *   Q x P / 8 bytes of candidate bits + Q x P / 8 bytes of hit bits + Q x P x 8 bytes of exact scores (written at
 *   candidate slots only) + Q x C x 16 bytes of chunk counts and prefixes + Q x 12 bytes of cuts and query norms, each
 *   array rounded up to 256 bytes: 8.25 bytes per (query, slot). */
size_t vm_range_workspace_bytes(const vm_memory *mem, int Q);
int vm_range_cosine(vm_memory *mem, const void *queries, int Q, double min_score, int score_mode,
                    const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride, int64_t row_offset,
                    int64_t max_hits, int64_t *out_rows, double *out_scores, int64_t *out_counts,
                    int64_t *out_rescored, void *workspace, size_t workspace_bytes, void *stream);
/* The same contract, exhaustive only: every live in-scope pair scored exactly, no fp32 scan (slow; tests, and a checker). */
int vm_range_cosine_exact(vm_memory *mem, const void *queries, int Q, double min_score, int score_mode,
                          const int64_t *scope_lo, const int64_t *scope_hi, int64_t row_stride, int64_t row_offset,
                          int64_t max_hits, int64_t *out_rows, double *out_scores, int64_t *out_counts,
                          void *workspace, size_t workspace_bytes, void *stream);
/* All-pairs exact cosine, out [Q, S] fp64: the post-compression filter of
 * src/pipeline/retriever_hybrid.py:494-504 (query vs segment embeddings) and a checker for the scan.
 * rows [S, D] dtype need not live in a vm_memory.  dtype VM_F32 takes fp32 operands: an embedder that returns fp32
 * values (every OpenAI-compatible server does) is then scored on its UN-rounded vectors, as the reference scores them
 * (:497), so `>= compression_threshold` decisions cannot flip on a 16-bit rounding.
 * 16-bit operands: D a multiple of 8 (VM_ERR_UNSUPPORTED otherwise), any S; VM_F32: any D >= 1.  S == 0 is VM_OK and
 * writes nothing (rows and out may then be null, as the address of an empty device tensor is). */
int vm_cosine_exact(vm_ctx *ctx, const void *queries, int Q, const void *rows, int64_t S, int D, int dtype,
                    double *out, void *stream);
/* The k best columns of every row of an all-pairs score matrix (vm_cosine_exact's output), by the order relation of
 * vm_topk_cosine: (score descending, column ascending).  scores [Q,S] fp64; col_limit (device int64 [Q], may be NULL):
 * query q ranks only columns < col_limit[q].  col_limit is clamped to [0, S]: a negative limit admits no column (all
 * -1 / 0.0), a limit above S admits all S, NULL means S for every query.  Equal scores (+0.0 and -0.0 are equal) come out
 * in column order and every returned score keeps the bits of its own entry; +-inf entries rank like any other value; NaN
 * is undefined, as in the reference.  k may exceed S.  out_rows = row_base + column, -1 / 0.0 padded.  With vm_cosine_exact
 * and vm_topk_merge this ranks the frames of a look-ahead group against the group's own EARLIER chunks, rows that are
 * about to be appended: what the reference's chunk-by-chunk loop would have stored by the time each chunk is searched
 * (src/pipeline/vlm_extractor.py:44-74; the same stable sort as src/components/pre_llm_injector.py:369). */
int vm_topk_select(vm_ctx *ctx, const double *scores, int Q, int64_t S, const int64_t *col_limit, int k,
                   int64_t row_base, double *out_scores, int64_t *out_rows, void *stream);
/* Merge `parts` per-shard results (each [Q,k], sorted as above, -1 padded) into the global top-k:
 * the step after the RCCL all-gather (and the cross-query max-merge input of pre_llm_injector.py:238-249).
 * scores [parts,Q,k] fp64, rows [parts,Q,k] int64.  Entries with row < 0 are padding and are dropped; the rest is ordered
 * by (score descending, row ascending) and the first k are kept, -1 / 0.0 padded.  Callers merge DISJOINT row sets (the
 * shards of a memory; the memory and a look-ahead group): the merge does not de-duplicate.  A (score, row) pair that
 * occurs in two parts comes out twice, the copies adjacent, the earlier part's first. */
int vm_topk_merge(vm_ctx *ctx, const double *scores, const int64_t *rows, int parts, int Q, int k,
                  double *out_scores, int64_t *out_rows, void *stream);

/* ---- measurement ---------------------------------------------------------------------------------------
 * Optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg; the
 * reference's counterpart is MetricsTracker.record_timing, src/core/metrics.py:18-24).  While enabled, every
 * kernel launch of this context is bracketed by two events from a preallocated pool (no sync, no allocation);
 * vm_profile_read synchronises the device, folds the pool into per-category totals and clears it.
 * Not capturable into a hipGraph while enabled. */
enum vm_prof_cat {
    VM_PROF_PREPROCESS = 0, VM_PROF_GEMM_PATCH, VM_PROF_GEMM_QKV, VM_PROF_GEMM_ACT, VM_PROF_GEMM_RESID,
    VM_PROF_ATTENTION, VM_PROF_LAYERNORM, VM_PROF_POOL, VM_PROF_APPEND, VM_PROF_TOPK_SCAN, VM_PROF_TOPK_FINALIZE,
    VM_PROF_TOPK_EXACT, VM_PROF_TOPK_MERGE,
    VM_PROF_GEMM_CLS,   /* the last encoder layer's GEMMs over the CLS rows only (one row per frame) */
    VM_PROF_NCAT
};
int vm_profile_enable(vm_ctx *ctx, int max_events);   /* 0 disables and frees the pool */
int vm_profile_read(vm_ctx *ctx, double *total_ms_host /*[VM_PROF_NCAT]*/, int64_t *launches_host /*[VM_PROF_NCAT]*/);
/* Restrict event recording to the categories whose bit (1u << vm_prof_cat) is set (default: all).  Two event
 * records cost several microseconds per launch on this stack, so a timed run enables only the kernel it reports. */
int vm_profile_mask(vm_ctx *ctx, uint32_t category_mask);

/* What this GPU sustains on 16-bit MFMA work, measured here and now (bench.py's `mfma_ceiling`).  The
 * chip lowers its clock under matrix load, so the 2.5 PFLOP/s of the data sheet is not what any kernel can reach on
 * random operands; these loops put a number on what can.  Runs back-to-back launches of a synthetic loop for about
 * `seconds` on `stream`, synchronises, and writes the mean rate in TFLOP/s to *tflops_host.
 *   variant 0: register-only v_mfma_f32_16x16x32_f16 loop with the operand pattern of a 128 x 64 wave tile, two waves
 *              per SIMD on every CU - no LDS, no memory;
 *   variant 1: + the fragment reads of the 256 x 256 GEMM tile (12 conflict-free ds_read_b128 per 32 MFMAs);
 *   variant 2: + its staging (4 KiB of LDS-DMA per wave and 32 MFMAs out of an L2-resident buffer, counted wait):
 *              the GEMM's K loop with no epilogue, barrier, tile boundary, miss or store.
 * zero_operands = 1 fills the operands with zeros (the same cycles at the clock an idle data path allows).
 * No reference counterpart (the reference has no kernels). */
int vm_probe_mfma(vm_ctx *ctx, int variant, int zero_operands, double seconds, double *tflops_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDMEM_H */
