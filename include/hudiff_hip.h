/*
 * hudiff_hip.h -- C ABI of libhudiff_hip.so: HuDiff's denoiser forward + T-step sampling loop on
 * MI355X (gfx950), hand-written HIP.  This is the drop-in boundary for ONE path of the reference:
 *
 *   reference interface replaced                          (file:line under /root/reference)
 *   ------------------------------------------------------------------------------------------------
 *   model_selected(config)  -> nn.Module                   utils/train_utils.py:43-55
 *   model.load_state_dict(ckpt['model'])                   antibody_scripts/sample.py:456-458
 *                                                          nanobody_scripts/nanosample.py:252-288
 *   model(H_L_seq, H_L_region_type, H_L_chn_type)          model/encoder/model.py:366-384
 *        -> logits[B, L, n_tokens]                         model/nanoencoder/model.py:325-343
 *   the sampling loop (forward, softmax[:, i, :22],        antibody_scripts/sample.py:499-513
 *        torch.multinomial, tokens[:, i] = s)              nanobody_scripts/nanosample.py:316-329
 *
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.  Every function returns an
 * HdStatus (0 = ok); hd_last_error() gives the message of the last failure on the calling thread.
 * A handle is bound to one device and one HIP stream and is NOT re-entrant; use one handle per GPU.
 * All tensors are caller-owned host memory unless a name ends in _dev; nothing is retained after return
 * (except by hd_load_tensor, which copies).
 *
 * Row / slot conventions: L = cfg.max_len IMGT slots per row (291 = 152 heavy + 139 light for the
 * antibody model, 152 for the nanobody model); tokens in [0,22] (utils/tokenizer.py:55-62: 20 residues,
 * X=20, '-'=21, <msk>=22); region in [0, n_region); chain type in {0 (H), 1 (L), 2 (K)} laid out as
 * chain[0:B] = heavy rows, chain[B:2B] = light rows (sample.py:172-176).
 *
 * Noise ("what makes sampled ids bit-exact under a fixed seed"):
 *   sampling  s = argmax_j softmax(logits[slot, 0:22])_j / q_j   (first maximum wins), q ~ Exp(1).
 *             q is either injected (q_noise) or generated:  Philox4x32-10, key = seed,
 *             counter = (j >> 2, global_row, step, 0xFFFFFFFF), word j & 3,
 *             u = ((w >> 8) + 0.5) * 2^-24,  q = -log(u).
 *   dropout   (the reference runs F.dropout with training=True at inference whenever cfg.dropout > 0,
 *             model/encoder/model.py:176-178, 295-303): keep-mask either injected or generated:
 *             (k0, k1) = Philox4x32-10(counter = (0, 0, step, site), key = seed)[0:2],
 *             rk = mix32(k0 ^ mix32(global_row + k1)),  w = mix32(rk + (slot * width + feature) * 0x9E3779B9),
 *             keep <=> w >= floor(p * 2^32);  kept values are scaled by 1/(1-p).
 *             site = layer for the token encoder (p = cfg.dropout), 64 + layer for Dual/NanoConv (p = 0.5).
 *             mix32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16.
 *   global_row = row0 + b, so results do not depend on how rows are sharded over GPUs.
 *   guided    (hd_set_guide, "guided sampling" below): the softmax is taken over g_j = (logits_j + bias_j) / temperature of the allowed
 *             tokens j; q is EXACTLY the noise of the unguided draw -- the same Philox counter or the same q_noise entry for all 22
 *             lanes, allowed or not -- and a token that is not allowed enters the argmax with -inf.  temperature == 0 (greedy) reads
 *             and generates no noise.
 *   block     (hd_set_slots_per_step, "block decoding" below): everything keyed by `step` in the draw -- the Philox counter word, the
 *             q_noise entry, the guide, target and logp -- stays keyed by the ORDER POSITION t, whatever K is; generated dropout
 *             masks of forward f are keyed by step = f * K, the forward's first position.
 *   confident (hd_set_slot_policy, "slot policy" below): the session itself permutes order[b, :] forward by forward; the draw at
 *             position t then meets the noise of position t exactly as above, at the slot the permuted order holds there.
 */
#ifndef HUDIFF_HIP_H
#define HUDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HD_ABI_VERSION 1      /* layout of HdConfig; rounds 4-5 added entry points only (hd_set_precision, hd_precision_report, hd_precision_reset,
                                 hd_set_option, hd_get_option, hd_debug_scatter_lnsync), likelihood scoring added hd_sample_logp, hd_score_begin,
                                 hd_score and the flag HD_RECORD_LOGP; the variant tests added hd_debug_launch_tally; guided sampling added hd_set_guide and
                                 the struct HdGuide; block decoding added hd_set_slots_per_step; the slot policy added hd_set_slot_policy and
                                 hd_sample_order; truncated sampling added hd_set_truncation and the struct HdTruncation; beam search added hd_set_beam and
                                 hd_beam_state; the mutation budget added hd_set_budget, hd_mutation_count and the struct HdBudget; the confidence
                                 threshold added hd_set_confidence, hd_sample_run_to_end, hd_sample_progress, hd_sample_forwards and hd_sample_keys; the
                                 distribution record added hd_sample_dist and the flag HD_RECORD_DIST; refinement rounds added hd_set_refine and
                                 hd_refine_state -- entry points only, so the version is unchanged */

typedef enum HdStatus {
    HD_OK = 0,
    HD_ERR_INVALID = 1,      /* bad argument / value out of range (token, region, chain, L, ...) */
    HD_ERR_UNSUPPORTED = 2,  /* configuration outside what the kernels implement                 */
    HD_ERR_STATE = 3,        /* call order (e.g. forward before finalize, missing tensors)       */
    HD_ERR_HIP = 4,          /* a HIP runtime call failed; message has the hipError string       */
    HD_ERR_NO_DEVICE = 5,    /* no usable gfx950 device: the product path never falls back to CPU */
    HD_ERR_NUMERIC = 6       /* hd_sample / hd_sample_end: a visited row had NaN / infinite logits at some step (the
                                reference's torch.multinomial raises there, sample.py:512); tokens are still returned */
} HdStatus;

enum { HD_KIND_ANTIBODY = 0, HD_KIND_NANOBODY = 1 };
enum { HD_ACT_RELU = 1, HD_ACT_GELU = 2 };

/* flags for hd_forward / hd_sample */
enum {
    HD_DROPOUT_FAITHFUL = 0u,  /* default: dropout active iff cfg.dropout > 0, generated masks      */
    HD_DROPOUT_OFF      = 1u,  /* sites are identity                                                */
    HD_DROPOUT_INJECT   = 2u,  /* caller supplies keep-masks (parity tests)                         */
    HD_DROPOUT_MASK     = 3u,
    HD_NO_GRAPH         = 4u,  /* launch kernels eagerly instead of replaying the captured hipGraph */
    HD_NO_PRUNE         = 8u,  /* hd_sample: evaluate the last attention block for every row (as hd_forward
                                  does) instead of only for the row each sequence visits at that step      */
    HD_ONE_LANE         = 16u, /* hd_sample: keep the batch on one stream (default: batches >= 16 rows are
                                  split into two halves that run concurrently on two streams)              */
    HD_LOOP_GRAPH       = 32u, /* hd_sample / hd_sample_run: the whole T-step loop of a lane is ONE hipGraph (a chain
                                  of T child-graph nodes of the captured step) launched once, instead of T replays
                                  of the step graph (same results; measured 2.4 % slower on MI355X) */
    HD_RECORD_LOGP      = 64u, /* hd_sample / hd_sample_begin: the session records the log-probability of every token it writes
                                  (hd_sample_logp); the drawn tokens are the same with and without the flag             */
    HD_RECORD_DIST      = 128u /* hd_sample / hd_sample_begin / hd_score_begin / hd_score: the session keeps the whole 22-token
                                  distribution of every draw ("distribution record", hd_sample_dist); a sampling session with it
                                  records logp too; tokens, logp and order are the same with and without the flag        */
};

/* Hyper-parameters: the `model:` section of configs/antibody_train.yml:3-24 / heavy_train.yml:3-21,
 * i.e. what sample.py reads from ckpt['config'|'pretrain_config'].model. */
typedef struct HdConfig {
    int32_t abi_version;       /* HD_ABI_VERSION */
    int32_t kind;              /* HD_KIND_* */
    int32_t n_tokens;          /* 23 */
    int32_t max_len;           /* 291 | 152 */
    int32_t h_len;             /* heavy slots: 152 (antibody: light = max_len - h_len) ; nanobody: max_len */
    int32_t d_model;           /* 256  (= d_embedding = s_model = r_model = n_pos_model) */
    int32_t sum_d_model;       /* 768 | 512 */
    int32_t n_encoder_layers;  /* 6 */
    int32_t dual_layers;       /* 6 */
    int32_t kernel_size;       /* 7 */
    int32_t r;                 /* 128: dilation of layer n = 2^(n mod (log2(r)+1)) */
    int32_t att_model;         /* 512 */
    int32_t nhead;             /* 8  (att_model / nhead must be 64) */
    int32_t dim_feedforward;   /* 256 */
    int32_t cs_layers;         /* 5 */
    int32_t n_region;          /* 7 */
    int32_t r_embedding;       /* 4 */
    int32_t n_side;            /* 3 (antibody only) */
    int32_t s_embedding;       /* 4 (antibody only) */
    int32_t enc_act;           /* HD_ACT_*: config.activation (token encoder)                        */
    int32_t conv_act;          /* HD_ACT_*: relu for DualConv (model.py:345), gelu for NanoConv       */
    float   dropout;           /* config.dropout */
} HdConfig;

typedef struct HdModel HdModel;

/* ---- construction (replaces model_selected + load_state_dict) ---------------------------------- */
int hd_device_count(void);
HdStatus hd_create(const HdConfig* cfg, int device, HdModel** out);
/* One call per state_dict entry, `key` = the reference's own key, data = float32 in
 * the torch layout ([out,in] Linear, [out,in,k] Conv1d).  The checkpoint's buffers are used when given:
 * 'pos_encoder.pos_embedding.pe' [L,1,d] and '...rope' (complex64 [L,32] passed as float32 [L,32,2],
 * identical in every layer); when absent they are recomputed.  Unknown keys -> HD_ERR_INVALID (strict). */
HdStatus hd_load_tensor(HdModel* m, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Checks every required key was loaded with the right shape, re-lays weights for the kernels and uploads. */
HdStatus hd_finalize(HdModel* m);
void hd_destroy(HdModel* m);
const char* hd_last_error(void);

/* ---- one denoiser forward (replaces model(tokens, region, chain)) -------------------------------
 * logits: [B, L, 23] float32.  chain: [2B] (antibody) or NULL (nanobody).
 * enc_masks [n_encoder_layers, B, L, d_model], conv_masks [dual_layers, B, L, sum_d_model] uint8
 * (1 = keep) are read only with HD_DROPOUT_INJECT.  seed/row0/step key generated masks. */
HdStatus hd_forward(HdModel* m, const int32_t* tokens, const int32_t* region, const int32_t* chain,
                    int32_t B, uint32_t flags, uint64_t seed, uint64_t row0, uint32_t step,
                    const uint8_t* enc_masks, const uint8_t* conv_masks, float* logits);

/* ---- the whole T-step sampling loop (replaces sample.py:499-513) --------------------------------
 * tokens [B, L] in/out.  order [B, Tmax]: slot visited by row b at step t; T [B]: steps of row b
 * (rows with t >= T[b] are left untouched at step t; T[b] == 0 is allowed).
 * q_noise [Tmax, B, 22] or NULL.  With HD_DROPOUT_INJECT: enc_masks [Tmax, n_enc, B, L, d],
 * conv_masks [Tmax, n_conv, B, L, D]. */
HdStatus hd_sample(HdModel* m, int32_t* tokens, const int32_t* region, const int32_t* chain,
                   const int32_t* order, const int32_t* T, int32_t B, int32_t Tmax, uint32_t flags,
                   uint64_t seed, uint64_t row0, const float* q_noise,
                   const uint8_t* enc_masks, const uint8_t* conv_masks);

/* Split form of hd_sample so that a caller can time the device-resident part:
 *   begin : validates, uploads inputs, computes the token-independent embedding branch
 *   run   : enqueues steps [t0, t1) on the handle's stream and returns without synchronising
 *   end   : synchronises and copies the tokens back                                                  */
HdStatus hd_sample_begin(HdModel* m, const int32_t* tokens, const int32_t* region, const int32_t* chain,
                         const int32_t* order, const int32_t* T, int32_t B, int32_t Tmax, uint32_t flags,
                         uint64_t seed, uint64_t row0, const float* q_noise,
                         const uint8_t* enc_masks, const uint8_t* conv_masks);
HdStatus hd_sample_run(HdModel* m, int32_t t0, int32_t t1);
/* Restores the tokens to their state at hd_sample_begin (device-to-device) and re-keys the noise with a new
 * seed, so that the same resident batch can be sampled again (independent replicas; bench.py). */
HdStatus hd_sample_restart(HdModel* m, uint64_t seed);
HdStatus hd_sample_end(HdModel* m, int32_t* tokens);
HdStatus hd_sync(HdModel* m);
/* Copies the tokens of the open session as they stand after the steps enqueued so far (synchronises; the session stays open):
 * lets a caller that restarts one resident batch many times keep every sample's result (bench.py: token agreement between
 * precision routes over all timed samples).  A guard that fired (see "precision routes") makes this fail with HD_ERR_STATE --
 * only hd_sample_end repeats a sample. */
HdStatus hd_sample_tokens(HdModel* m, int32_t* tokens);

/* ---- likelihood scoring ---------------------------------------------------------------------------
 * The draw stage of a step is the only place where the step's distribution p = softmax(logits[slot, 0:22]) exists.  A RECORDING
 * session (HD_RECORD_LOGP) keeps, for row b at step t < T[b], the log-probability of the token s it wrote there,
 *     logp[b, t] = (logit_s - max_j logit_j) - log(sum_j exp(logit_j - max_j logit_j))        (fp32, from the logits, not log(p)),
 * under the distribution the token was drawn from (so under the dropout masks of that step when dropout is active).
 *
 * hd_sample_logp copies logp [B, Tmax] of the session out, rows in whole-batch order whatever the lane split; entries with
 * t >= T[b] are 0 (so are steps not run yet).  Legal inside an open session -- it synchronises, and fails with HD_ERR_STATE after a
 * guard has fired, like hd_sample_tokens -- and after hd_sample / hd_sample_end until the next hd_sample_begin / hd_score_begin /
 * hd_forward / hd_destroy.  A session that did not record -> HD_ERR_STATE.  The range guard and the ln_sync guard repeat a
 * recording session like any other; the values then come from the repeat.
 *
 * hd_score_begin opens a TEACHER-FORCED recording session on sequences the caller already has: `tokens` [B, L] are complete,
 * the library takes target[b, t] = tokens[b, order[b, t]] for t < T[b] (a target outside [0, 21] -> HD_ERR_INVALID), masks those
 * slots to 22 in its own copy, and every step writes its target instead of drawing: no noise is read or generated, and
 * logp[b, t] = log p(target | the slots that are not masked at step t).  sum_t logp[b, t] is the order-agnostic log-likelihood
 * of the scored slots along the ONE visiting order given (the quantity the network was trained on is its mean over orders).
 * hd_sample_run, hd_sample_restart, hd_sync, hd_sample_end (returns the re-filled tokens = the input), hd_sample_tokens,
 * hd_last_run_ms and hd_sample_logp work on that session as on a sampling one; dropout flags, seed / row0 (generated masks) and
 * injected masks mean what they mean for hd_sample.  hd_score = begin + run(0, Tmax) + end + hd_sample_logp.
 *
 * In a GUIDED session ("guided sampling" below) logp is the log-probability under the guided distribution:
 *     logp[b, t] = (g_s - max_j g_j) - log(sum_j exp(g_j - max_j g_j)),  j over the allowed tokens,
 * of the drawn token in a recording session and of the target in a scoring one (a target that is not allowed -> HD_ERR_INVALID at
 * hd_score_begin; so is temperature == 0).  A greedy session (temperature == 0) records the log-probability of its token under
 * the temperature-1 guided distribution.
 *
 * In a TRUNCATED session ("truncated sampling" below) logp is the log-probability under the truncated distribution (the sum runs over
 * the kept tokens only).  A SCORING session may then return -inf: a target that the cut of its step removes has probability 0 under
 * this sampler, logp[b, t] = -inf, the target is still written, and neither an error nor the numeric flag is raised. */
HdStatus hd_sample_logp(HdModel* m, float* logp /* [B, Tmax] */);
HdStatus hd_score_begin(HdModel* m, const int32_t* tokens, const int32_t* region, const int32_t* chain,
                        const int32_t* order, const int32_t* T, int32_t B, int32_t Tmax, uint32_t flags,
                        uint64_t seed, uint64_t row0, const uint8_t* enc_masks, const uint8_t* conv_masks);
HdStatus hd_score(HdModel* m, const int32_t* tokens, const int32_t* region, const int32_t* chain,
                  const int32_t* order, const int32_t* T, int32_t B, int32_t Tmax, uint32_t flags,
                  uint64_t seed, uint64_t row0, const uint8_t* enc_masks, const uint8_t* conv_masks, float* logp /* [B, Tmax] */);

/* ---- guided sampling ------------------------------------------------------------------------------
 * A guide steers the draw stage of every visited slot of every row of ONE session, sampling or scoring.  For row b visiting slot s
 * with raw logits z[0:22]:
 *     g_j   = (z_j + bias[b, s, j]) / temperature     for the tokens j allowed at (b, s)            (fp32)
 *     g_j   = -inf                                    for the others
 *     p     = softmax(g) over the allowed j
 *     token = argmax_j p_j / q_j                      (lowest index wins; a token that is not allowed enters with -inf, so an allowed
 *                                                      one whose p underflowed to 0 still beats it)
 *     logp  = (g_token - max g) - log(sum_j exp(g_j - max g))
 * allow[b, s] is a uint32 whose bit j (0..21) allows token j; q is exactly the noise of the unguided draw (see "Noise").  With all 22
 * bits set, no (or zero) bias and temperature == 1, g_j == z_j bit for bit and the session produces the tokens and the recorded
 * log-probabilities of an unguided one bit for bit.  temperature == 0 is the greedy decode: token = argmax_j (z_j + bias_j) over the
 * allowed j (lowest index wins), no noise is read or generated, and logp is that token's log-probability under the temperature-1
 * guided distribution.  HD_ERR_NUMERIC is raised from the guided sum exactly as from the raw one.
 *
 * Lifetime: hd_set_guide copies the arrays (nothing of the caller's is retained).  The guide applies to the NEXT hd_sample_begin /
 * hd_sample / hd_score_begin / hd_score on the handle, and that call consumes it whether it succeeds or fails: the session after it
 * is unguided unless a guide is set again.  Inside its session the guide stays: hd_sample_restart keeps it, and so do the range guard
 * and the ln_sync guard when they repeat a call.  hd_forward neither uses nor clears it.  NULL clears a guide not yet consumed.
 * Inside an open session -> HD_ERR_STATE; a NULL handle -> HD_ERR_INVALID.
 *
 * HD_ERR_INVALID at hd_set_guide: a temperature that is not finite, negative, or non-zero outside [0.01, 100]; a bias value that is
 * not finite (forbid a token through `allow`).  At the begin: B differs from the session's; a VISITED slot (b, order[b, t]), t < T[b],
 * has no allowed token among bits 0..21; in a scoring session a target that is not allowed at its slot, or temperature == 0.  Slots
 * that are not visited are never checked and never read. */
typedef struct HdGuide {
    int32_t B;              /* rows the arrays describe; must equal B of the session that consumes it */
    float temperature;      /* 0 = greedy, else in [0.01, 100] */
    const uint32_t* allow;  /* [B, L] or NULL = everything allowed */
    const float* bias;      /* [B, L, 22] or NULL */
} HdGuide;
HdStatus hd_set_guide(HdModel* m, const HdGuide* g);   /* NULL clears */

/* ---- block decoding -------------------------------------------------------------------------------
 * A session has a block size K, its "slots per step" (default 1 = one slot per denoiser forward, the loop of the reference).  With
 * K > 1, forward number f = 0, 1, ... runs the denoiser ONCE on the current tokens and handles the K order positions t = f * K + j,
 * j = 0 .. K-1: for every row b with t < T[b] it does what step t of a one-slot session does at slot = order[b, t] -- draws (or, when
 * scoring, writes the target), writes tokens[b, slot], records logp[b, t] -- but from the hidden row of THIS forward, so the slots of
 * one group do not see each other.  A row takes ceil(T[b] / K) forwards instead of T[b]; the price is that known approximation.
 *
 * Keys: position t meets exactly the noise and the guide it meets at K = 1 (see "Noise": Philox counter word `step` = t,
 * q_noise[t, row, :], the guide of (b, order[b, t]), target[b, t], logp[b, t]).  Generated dropout masks of forward f are keyed by
 * step = f * K.  The recorded log-probabilities are therefore the exact log-likelihood of the session's tokens under the block
 * sampler, and a scoring session with the same K, order and guide reproduces them.  The forward of a block session evaluates the
 * last attention block for every row (as HD_NO_PRUNE and hd_forward do); K = 1 is the one-slot session: the same launches, the same
 * bits.
 *
 * Lifetime: the block size applies to the NEXT hd_sample_begin / hd_sample / hd_score_begin / hd_score on the handle, and that call
 * consumes it whether it succeeds or fails: the session after it has K = 1 unless a block size is set again.  Inside its session the
 * block size stays: hd_sample_restart keeps it, and so do the range guard and the ln_sync guard when they repeat a call.  hd_forward
 * neither uses nor clears it.  Inside an open session -> HD_ERR_STATE; a NULL handle, or k outside [1, 64] -> HD_ERR_INVALID.
 *
 * At the begin, with K > 1 only: a row whose order repeats a slot inside one group order[b, f*K : min(f*K + K, T[b])] ->
 * HD_ERR_INVALID (two workgroups would write one token; the same order stays legal at K = 1); HD_DROPOUT_INJECT ->
 * HD_ERR_UNSUPPORTED (injected masks are laid out per step of a one-slot loop; generated dropout and dropout off work).
 *
 * hd_sample_run(t0, t1) keeps taking ORDER POSITIONS: t0 must be a multiple of K, t1 a multiple of K or equal to Tmax, anything else
 * -> HD_ERR_INVALID; it enqueues ceil((t1 - t0) / K) forwards.  hd_last_run_ms keeps reporting t1 - t0 in `steps`: the number of
 * forwards timed is ceil(steps / K). */
HdStatus hd_set_slots_per_step(HdModel* m, int32_t k);

/* ---- slot policy ----------------------------------------------------------------------------------
 * A session has a slot policy: WHICH slots a forward fills.  HD_SLOTS_GIVEN (default) follows order[b, :] as the caller wrote it.
 * HD_SLOTS_CONFIDENT, for any block size K in [1, 64], lets the device pick, forward by forward, the K remaining slots of each row
 * whose distribution is most peaked, from the hidden rows of that very forward.  order[b, 0:T[b]] is then the row's CANDIDATE LIST:
 * the slots to fill, and the tie-break.
 *
 * Forward f, row b, n = min(f * K, T[b]) positions already visited:
 *   1. for every remaining position i in [n, T[b]), slot s = order[b, i], the 22 values g_j are formed from this forward's hidden row
 *      exactly as the draw forms them: the raw logits in an unguided session; (z_j + bias_j) / temperature over the allowed tokens in
 *      a guided one and -inf for the others, with divisor 1 at temperature 0;
 *   2. the key is c_i = sum_j exp(g_j - max_j g_j) in fp32 (= 1 / max_j p_j: smaller is more confident); a key that is not a finite
 *      positive number ranks behind every finite one;
 *   3. the min(K, T[b] - n) positions with the smallest (c_i, i), compared lexicographically, are chosen and become, in ascending
 *      (c_i, i), positions n, n + 1, ... of the row's order; the positions not chosen follow in their previous relative order (a
 *      stable partition).  What is keyed by order position -- the target of a scoring session, the guide's allowed bits and bias --
 *      moves with its entry.  Entries at t >= T[b] are never touched;
 *   4. the forward's draw then runs as in a given-order block session on the permuted order: position t draws at order[b, t] with the
 *      noise, guide, target and logp[b, t] of position t.
 * The selection runs on the device inside the captured step (two launches in front of the draw); nothing is read back.  The forward of
 * a confident session evaluates the last attention block for every row, at K = 1 too.  Dropout masks, hd_sample_run(t0, t1)
 * granularity and hd_last_run_ms are those of "block decoding".
 *
 * Consequences.  Replay: a HD_SLOTS_GIVEN session with the same K, seed or q_noise, row0, guide and dropout mode, given the realised
 * order hd_sample_order returns, draws the same tokens and records the same logp bit for bit.  The selection is a deterministic
 * function of the state, so sum_t logp[b, t] of a recording session is the exact log-likelihood of its tokens under this sampler.  A
 * scoring session (hd_score_begin) consumes the policy too: teacher-forced, the library picks the order and writes the targets, and
 * scoring a confident session's tokens from the same candidate list, K, guide and dropout key reproduces its realised order.
 *
 * Lifetime: as the block size -- the policy applies to the NEXT hd_sample_begin / hd_sample / hd_score_begin / hd_score, which
 * consumes it whether it succeeds or fails; hd_sample_restart (which puts the candidate list back) and the guards' repeats keep it;
 * hd_forward neither uses nor clears it.  hd_set_slot_policy: NULL handle or a value outside {0, 1} -> HD_ERR_INVALID; inside an open
 * session -> HD_ERR_STATE.  At the begin, confident sessions only: a row whose order[b, 0:T[b]] repeats a slot anywhere ->
 * HD_ERR_INVALID (the list is a set; the same order stays legal under HD_SLOTS_GIVEN at K = 1); HD_DROPOUT_INJECT ->
 * HD_ERR_UNSUPPORTED.
 *
 * hd_sample_order copies the current order [B, Tmax] of the session out, rows in whole-batch order whatever the lane split: positions
 * < min(steps run, T[b]) -- in a threshold session ("confidence threshold"): positions < filled[b] -- are the visited slots in
 * visiting order; in a HD_SLOTS_GIVEN session it is the order that was given.  Legal
 * where hd_sample_logp is: inside an open session (it synchronises; HD_ERR_STATE after a guard has fired) and after hd_sample /
 * hd_sample_end until the next begin, hd_forward or hd_destroy.  No session ever opened, or a NULL handle -> HD_ERR_STATE. */
enum { HD_SLOTS_GIVEN = 0, HD_SLOTS_CONFIDENT = 1 };
HdStatus hd_set_slot_policy(HdModel* m, int32_t policy);
HdStatus hd_sample_order(HdModel* m, int32_t* order /* [B, Tmax] */);

/* ---- truncated sampling ---------------------------------------------------------------------------
 * A session may carry a truncation (top_k, top_p, min_p): a cut of the 22-token distribution of every draw, applied in the draw stage
 * in front of the draw.  For row b at order position t let g_j, j = 0..21, be exactly the values the draw forms without it: the raw
 * logits in an unguided session; (z_j + bias_j) / temperature over the allowed tokens of a guided one (divisor 1 at temperature 0);
 * -inf for a token that is not allowed.  With mx = max_j g_j:
 *     e_j      = expf(g_j - mx) for allowed j, 0 otherwise                  (fp32, as without truncation)
 *     esum     = sum_j e_j                                                  (the same reduction; HD_ERR_NUMERIC is still raised from THIS sum)
 *     rank_j   = #{ i allowed : g_i > g_j  or (g_i == g_j and i < j) }      (ranking is on g, not on e: expf can merge distinct g)
 *     before_j = sum of e_i over the i with rank_i < rank_j, accumulated in ascending token index i, fp32
 *     keep_j   = allowed_j
 *                and (top_k off  or rank_j < top_k)
 *                and (top_p off  or before_j < top_p * esum)                (the smallest head whose mass reaches top_p)
 *                and (min_p off  or e_j >= min_p)                           (e of the best token is exactly 1: p_j >= min_p * p_max)
 *     the rank-0 token is always kept
 *     esum'    = sum_j (keep_j ? e_j : 0)                                   (same reduction order)
 *     p'_j     = e_j / esum' for kept j; a token that is not kept enters the argmax with -inf
 *     token    = argmax_j p'_j / q_j        q is EXACTLY the noise position t meets without truncation (see "Noise")
 *     logp     = (g_token - mx) - logf(esum')
 * top_k is off when it is 0 or >= 22, top_p when it is >= 1, min_p when it is 0.  With all three off the truncation is the same as
 * none: the library treats it as cleared and the session launches the kernels it launches without hd_set_truncation.  Valid ranges:
 * top_k in [0, 22]; top_p finite in (0, 1]; min_p finite in [0, 1]; anything else -> HD_ERR_INVALID.
 *
 * Greedy (temperature 0): the token is unchanged (the argmax is always kept), no noise is read, and logp is the token's under the
 * temperature-1 guided, truncated distribution.  Scoring: a target that is not kept gets logp[b, t] = -inf (see "likelihood scoring");
 * this cannot be known at the begin, whose checks stay as they are.  Confident slot policy: the key becomes c_i = esum' (= 1 / max p'),
 * formed with the same keep-set from the same forward; everything else of "slot policy", the replay property included, holds with the
 * same truncation on both sides.  Block sessions: the truncation acts per order position, like the guide.
 *
 * Lifetime: as the block size and the slot policy -- one-shot: the NEXT hd_sample_begin / hd_sample / hd_score_begin / hd_score
 * consumes it whether it succeeds or fails; hd_sample_restart and the guards' repeats keep it; hd_forward neither uses nor clears it.
 * NULL clears a truncation not yet consumed.  Inside an open session -> HD_ERR_STATE; a NULL handle -> HD_ERR_INVALID. */
typedef struct HdTruncation {
    int32_t top_k;          /* keep the top_k best tokens; 0 or >= 22 = off */
    float top_p;            /* keep the smallest head whose probability mass reaches top_p; in (0, 1], 1 = off */
    float min_p;            /* keep tokens with p >= min_p * p_max; in [0, 1], 0 = off */
} HdTruncation;
HdStatus hd_set_truncation(HdModel* m, const HdTruncation* t);   /* NULL clears */

/* ---- beam search ----------------------------------------------------------------------------------
 * A session may carry a beam width W in [1, 64]: it is then a SEARCH, not a sampler.  Its B = G * W rows are G groups of W consecutive
 * rows (rows g*W .. g*W+W-1 are group g), and the device keeps, position by position, the W best continuations of every group.
 * State per row: score[b] (fp32, the cumulative log-probability) and parent[b, t] (int32).  At the begin and at hd_sample_restart
 * score is 0 for the first row of each group and -inf ("dead") for the others; parent is 0.
 *
 * Order position t of group g, for t < T (a group with t >= T is left untouched):
 *   1. one denoiser forward, as in a one-slot session (the pruned tail applies: every row visits order[b, t]);
 *   2. candidates: for every row b of the group g_j, mx, e_j, esum, the keep-set and esum' are formed exactly as the draw stage forms
 *      them for an unguided, guided or truncated session (same arithmetic, same reduction order; HD_ERR_NUMERIC from the full sum), then
 *          lp[b, j]   = (g_j - mx) - logf(esum')   for a kept token, -inf for a token that is not allowed or not kept
 *          cand[b, j] = score[b] + lp[b, j]        (one fp32 add)
 *   3. selection: the W * 22 candidates (w, j) of the group are ranked by cand descending; ties go to the smaller (w, j), compared
 *      lexicographically; a candidate that is -inf or NaN ranks behind every finite one, in (w, j) order among its like;
 *   4. gather: the candidate of rank r < W becomes row g*W + r: its tokens are the parent row's with tokens[order[t]] = j,
 *      score = cand, parent[b, t] = w (the index inside the group), logp[b, t] = lp[w, j].
 * Rows therefore always stand in score order.  A dead row stays well formed: its tokens are valid, its score is -inf.  Steps 2-4 run
 * on the device inside the captured step (two launches in the place of the draw); nothing is read back and no noise is read or
 * generated.  The selection is a function of the candidate table alone: a session repeats bit for bit.
 *
 * A beam session always records, whatever HD_RECORD_LOGP says: hd_sample_logp returns the raw logp[b, t] above, the step value of the
 * candidate row b became at position t; it is NOT permuted by later steps (follow `parent` backwards to read a final row's history).
 * hd_beam_state copies score [B], parent [B, Tmax] and cand [B, 22] out (each pointer may be NULL), rows in whole-batch order whatever
 * the lane split; cand is the candidate table of the last position run (unspecified before the first).  Legal where hd_sample_logp is;
 * outside a beam session -> HD_ERR_STATE.
 *
 * Lifetime: as the block size -- one-shot: the NEXT hd_sample_begin / hd_sample consumes the width whether it succeeds or fails;
 * hd_sample_restart and the guards' repeats keep it (and start from the initial state again); hd_forward neither uses nor clears it.
 * Width 0 clears a width not yet consumed.  Inside an open session -> HD_ERR_STATE; a NULL handle or a width outside [0, 64] ->
 * HD_ERR_INVALID.
 *
 * At the begin: B % W != 0 -> HD_ERR_INVALID; a row that differs from the first row of its group in tokens, region, chain,
 * order[b, 0:T[b]] or T -> HD_ERR_INVALID; q_noise != NULL -> HD_ERR_INVALID; a guide with temperature 0 -> HD_ERR_INVALID (as for
 * scoring).  A guide and a truncation compose with the beam, both per order position as in a sampling session.  A block size > 1 or
 * HD_SLOTS_CONFIDENT -> HD_ERR_UNSUPPORTED; hd_score_begin / hd_score with a width pending consume it and return HD_ERR_UNSUPPORTED.
 * Dropout must be off (HD_DROPOUT_OFF, or cfg.dropout == 0), anything else -> HD_ERR_UNSUPPORTED: generated masks are keyed by row, so
 * the rows of a group would be ranked under different sub-networks.  Lanes are cut at group boundaries, balanced over groups, at
 * most G of them.  hd_sample_run(t0, t1) takes any 0 <= t0 < t1 <= Tmax, as at K = 1. */
HdStatus hd_set_beam(HdModel* m, int32_t width);   /* 0 clears */
HdStatus hd_beam_state(HdModel* m, float* score /* [B] */, int32_t* parent /* [B, Tmax] */, float* cand /* [B, 22] */);

/* ---- mutation budget ------------------------------------------------------------------------------
 * A session may carry a budget: row b may differ from its ORIGIN in at most max_mutations[b] of the slots it visits.  This is the one
 * option that depends on what the row has already drawn, so it has state: n[b], an int32 count of mutations so far, 0 at the begin and
 * at hd_sample_restart (so the guards' repeats start from 0 as well).
 *
 * Order position t of row b, with s = order[b, t], o = origin[b, s], M = max_mutations[b]:
 *   1. the row is EXHAUSTED at t iff o <= 21 and n[b] >= M.  The allowed set of the draw is then exactly {o}; otherwise it is the guide's
 *      set (all 22 tokens without a guide);
 *   2. everything else is the guided draw stage as it stands, on that allowed set and in the same arithmetic: g, mx, e, esum, the numeric
 *      flag, the cut, the noise of position t, the argmax, logp.  An exhausted draw writes o and records logp = +0.0f exactly
 *      (expf(0) = 1, logf(1) = 0); a greedy session (temperature 0) writes o;
 *   3. after the token is written: if o <= 21 and token != o, n[b] += 1;
 *   4. a free slot (o = 22) is never forced and never counted.
 * All of it runs on the device inside the captured step; nothing is read back.  A budgeted session always runs the guided form of the
 * draw, as a truncated one does (every bit set, no bias, temperature 1 when no guide is set), and a session whose rows never become
 * exhausted produces, bit for bit, the tokens, logp, order and beam state of the same session without a budget.
 *
 * Scoring (hd_score_begin / hd_score) consumes a budget too: the target is written as always; an exhausted position whose target is
 * not o records -inf, as a cut target does, and raises neither an error nor the numeric flag; rule 3 counts targets, so n may pass M.
 * Scoring a budgeted session's tokens under the same origin, budget, order, guide and dropout key reproduces its logp bit for bit.
 *
 * Beam: n is part of the row state.  The candidate table is formed exactly as without a budget, then lp[b, j] = cand[b, j] = -inf where
 * the row is exhausted and j != o.  lp[b, o] is NOT renormalised: the rows of one group have spent different amounts, and under a
 * renormalised score an exhausted row would pay nothing for the rest of the sequence, so the search would reward spending the budget
 * early.  The score of a beam row stays its log-likelihood under the guide alone; the budget is a feasibility constraint on candidates.
 * The gather carries n with the row: n of rank r = n[parent] + (j != o and o <= 21), read before any row of the group is overwritten.
 * o is always feasible, so a live row always has a finite candidate.
 *
 * Confident slot policy: the key of a remaining position is formed on the allowed set of rule 1, with n as it stands at the start of the
 * forward.  Every origin-bearing slot of an exhausted row then has the key exactly 1.0f, the smallest possible, so those slots are
 * taken first, in list order.
 *
 * Lifetime: as the guide -- hd_set_budget copies the arrays; one-shot: the NEXT hd_sample_begin / hd_sample / hd_score_begin / hd_score
 * consumes it whether it succeeds or fails; hd_sample_restart and the guards' repeats keep it; hd_forward neither uses nor clears it.
 * NULL clears a budget not yet consumed.  Inside an open session -> HD_ERR_STATE; a NULL handle, B <= 0 or a NULL array -> HD_ERR_INVALID.
 *
 * At the begin (only VISITED slots are checked or read, as for the guide): B differs -> HD_ERR_INVALID; a visited origin outside [0, 22]
 * or a negative max_mutations[b] -> HD_ERR_INVALID; a visited slot whose o <= 21 is not allowed there by the guide -> HD_ERR_INVALID (an
 * exhausted row must be able to draw); beam: a row whose max_mutations or visited origins differ from the first row of its group ->
 * HD_ERR_INVALID; beam together with a truncation -> HD_ERR_UNSUPPORTED (the cut may remove the only feasible token); slots per step
 * K > 1 -> HD_ERR_UNSUPPORTED (the K draws of one forward cannot see each other's count).
 *
 * hd_mutation_count copies n [B] out, rows in whole-batch order whatever the lane split.  Legal where hd_sample_logp is: inside a
 * session, where it synchronises, and after it until the next begin.  A session without a budget -> HD_ERR_STATE. */
typedef struct HdBudget {
    int32_t B;                      /* rows described; must equal B of the session that consumes it */
    const int32_t* origin;          /* [B, L]: token 0..21 = the residue a draw is compared with; 22 = the slot has no origin (free) */
    const int32_t* max_mutations;   /* [B], >= 0 */
} HdBudget;
HdStatus hd_set_budget(HdModel* m, const HdBudget* b);      /* NULL clears */
HdStatus hd_mutation_count(HdModel* m, int32_t* n /* [B] */);

/* ---- confidence threshold -------------------------------------------------------------------------
 * A confident session ("slot policy") may carry a threshold tau in (0, 1]: a forward then fills EVERY remaining slot of a row whose top
 * probability is at least tau -- at least one, at most K (hd_set_slots_per_step, now a cap).  The number of forwards follows the
 * model's certainty, row by row.  The host forms cmax = 1.0f / tau (one fp32 division); a key c = 1 / p_max qualifies iff c <= cmax.
 *
 * State per row, set at the begin and at every hd_sample_restart: filled[b], the positions of order[b, :] already drawn (0); cnt[b], the
 * count of the last forward (0); fwd[b, t], the forward number that drew position t (-1 where nothing was drawn).
 *
 * Forward number f, row b, n = filled[b], N = T[b] - n; a row with N <= 0 is left alone.  Otherwise:
 *   1. keys c_i of every remaining position i in [n, T[b]) exactly as in "slot policy" (guided, truncated and temperature-0 forms
 *      included); a key that is not a finite positive number becomes +inf;
 *   2. q = the number of remaining positions with c_i <= cmax (an fp32 compare; an infinite key never qualifies);
 *   3. cnt = min(K, N, max(1, q));
 *   4. the cnt smallest (c_i, i) move to positions n .. n + cnt - 1 in ascending order, the rest follow in their previous relative
 *      order, targets and guide entries move with their positions: the permutation of "slot policy" with cnt in place of min(K, N);
 *   5. position t = n + j, j < cnt, is drawn at order[b, t] with the noise, guide, target and logp[b, t] of position t ("block
 *      decoding"); then fwd[b, t] = f and filled[b] = n + cnt.
 * Generated dropout masks of forward f are keyed by step = f (a confident K-session keys them by f * K); the Philox counter word of a
 * draw stays the position t.  A row needs between ceil(T / K) and T forwards; Tmax forwards always finish every row.  All of it runs on
 * the device inside the captured step, in the launches of a confident session; a threshold session always runs the guided form of the
 * kernels, as a truncated one does (every bit set, no bias, temperature 1 when no guide is set).
 *
 * Running.  hd_sample_run(f0, f1) takes FORWARD NUMBERS in a threshold session: 0 <= f0 <= f1 <= Tmax, no multiple-of-K rule; it
 * enqueues f1 - f0 forwards without synchronising (each continues from the rows' progress; f names the dropout masks and fwd), and
 * hd_last_run_ms reports forwards in `steps`.  HD_LOOP_GRAPH works as elsewhere.  hd_sample_run_to_end(chunk, &forwards), legal in
 * threshold sessions only (HD_ERR_STATE elsewhere; chunk outside [1, Tmax] -> HD_ERR_INVALID), enqueues `chunk` forwards from where the
 * session stands, reads filled back (one small device-to-host copy and a synchronise; the guards are looked at as in hd_sync), and
 * repeats until every row has filled[b] == T[b] or Tmax forwards have run; `forwards` (may be NULL) gets the number it enqueued.
 * hd_sample and hd_score run a threshold session this way with chunk 4.  A guard's repeat in hd_sample_end finishes the rows again:
 * on the fp32 kernels the keys differ in their last bits and the rows may need a different number of forwards, so a session that was
 * run to its end is run to its end again by the repeat (any other repeats the same number of forwards).
 *
 * Consequences.  With every finite key qualifying (tau <= 1/22, since c <= 22) the session is the confident K-session: order, tokens
 * and logp agree bit for bit at dropout off, and fwd[b, t] = t / K.  With no key ever qualifying it is the confident 1-session for any
 * cap K, generated dropout included, and fwd[b, t] = t.  The selection is a deterministic function of the state, so a recording
 * session's row total is the exact log-likelihood of its tokens under this sampler.  A scoring session consumes the threshold too,
 * teacher-forced with the same rule: scoring a threshold session's tokens from the same list, K, tau, guide and dropout key reproduces
 * its order and fwd.
 *
 * Read-backs, legal where hd_sample_order is, rows in whole-batch order whatever the lane split, HD_ERR_STATE after a guard has fired
 * inside the session: hd_sample_progress copies filled [B] out and hd_sample_forwards fwd [B, Tmax] (a session without a threshold ->
 * HD_ERR_STATE).  hd_sample_keys works for ANY confident session, with or without a threshold: the keys [B, Tmax] of the last forward
 * run, indexed by order position as the order stood BEFORE that forward's permutation, meaningful for the positions [n, T[b]) of that
 * forward only (zeros before the first forward) -- the per-slot certainty map of a forward.  A HD_SLOTS_GIVEN session -> HD_ERR_STATE.
 *
 * Lifetime: as the block size -- one-shot: the NEXT hd_sample_begin / hd_sample / hd_score_begin / hd_score consumes the threshold
 * whether it succeeds or fails; hd_sample_restart and the guards' repeats keep it; hd_forward neither uses nor clears it.  tau == 0
 * clears a threshold not yet consumed.  tau not finite, negative or above 1, or a NULL handle -> HD_ERR_INVALID; inside an open
 * session -> HD_ERR_STATE.  At the begin: a threshold with HD_SLOTS_GIVEN -> HD_ERR_UNSUPPORTED; with a mutation budget ->
 * HD_ERR_UNSUPPORTED at any K; a beam is refused by the confident policy already, whose other checks (the candidate list is a set, no
 * injected dropout) stay. */
HdStatus hd_set_confidence(HdModel* m, float tau);          /* 0 clears */
HdStatus hd_sample_run_to_end(HdModel* m, int32_t chunk, int32_t* forwards /* may be NULL */);
HdStatus hd_sample_progress(HdModel* m, int32_t* filled /* [B] */);
HdStatus hd_sample_forwards(HdModel* m, int32_t* fwd /* [B, Tmax] */);
HdStatus hd_sample_keys(HdModel* m, float* conf /* [B, Tmax] */);

/* ---- distribution record --------------------------------------------------------------------------
 * A session begun with the flag HD_RECORD_DIST (hd_sample, hd_sample_begin, hd_score_begin, hd_score) keeps dist [B, Tmax, 22] float32:
 * the distribution every draw was taken from, or every target was scored under.  A sampling session with the flag records logp too, as
 * under HD_RECORD_LOGP.
 *
 * For row b at order position t < T[b] that a forward drew or scored, with g_j, mx = max g, esum and the allowed / kept sets as the draw
 * stage forms them -- after the guide ("guided sampling"), the temperature, the forced set of an exhausted budget ("mutation budget") and
 * the renormalisation of the cut ("truncated sampling"):
 *     dist[b, t, j] = (g_j - mx) - logf(esum)     if token j is allowed and kept
 *                   = -inf                         otherwise
 * the same three fp32 operations in the same order as logp[b, t].  Consequences:
 *   - dist[b, t, token written] == logp[b, t] bit for bit wherever that logp is finite;
 *   - where a scoring session records -inf (a target the cut removed, a mutation an exhausted budget no longer pays for) the target's
 *     entry is -inf too;
 *   - an exhausted budgeted draw has +0.0f at its origin and -inf at the 21 other tokens;
 *   - temperature 0 records the temperature-1 distribution, the one its logp is under;
 *   - entries with t >= T[b], or of positions not yet run, are 0; a row that raised the numeric flag has unspecified entries.
 * The index is the (b, t) of logp: with block decoding, the confident policy and the threshold, position t holds the distribution of the
 * entry the selection put there.  The stores happen inside the draw launch (lanes 0..21 of one wave, 88 contiguous bytes): a session
 * with the flag launches what it launches without it, and tokens, logp and order are the same bits.
 *
 * hd_sample_dist copies dist [B, Tmax, 22] out, rows in whole-batch order whatever the lane split.  Legal exactly where hd_sample_logp
 * is: inside an open session (it synchronises; HD_ERR_STATE after a guard has fired -- hd_sample_end repeats the sample and the values
 * read back then come from the repeat) and after hd_sample / hd_sample_end / hd_score until the next begin or hd_forward.  A session
 * without the flag -> HD_ERR_STATE.  hd_sample_restart zeroes the record.
 *
 * The flag with a beam width pending (hd_set_beam) -> HD_ERR_UNSUPPORTED: a beam session has its candidate table (hd_beam_state). */
HdStatus hd_sample_dist(HdModel* m, float* dist /* [B, Tmax, 22] */);

/* ---- refinement rounds ----------------------------------------------------------------------------
 * A sampling session may carry a refinement (rounds, R, below): after a row has drawn its whole list, the slots it was least sure about
 * are masked again and redrawn with everything else as context (mask-predict), `rounds` times.  rounds in [1, 16], R in [1, 64] slots per
 * round, below a finite float <= 0.  Such a session always records (as under HD_RECORD_LOGP); the tokens of its first pass are those of the
 * same session without refinement, bit for bit.
 *
 * A round is nothing but the device APPENDING order positions to a row.  State per row: T_now[b] (T[b] at the begin) and
 * rounds_done[b] (0).  At the start of every step, before the forward, with s the step (an order position; a multiple of K), a row with
 * s >= T_now[b] and rounds_done[b] < rounds opens a round:
 *   1. for every slot in order[b, 0:T_now[b]) (holes excluded, see 4) its LIVE position u is the last position holding that slot; a live
 *      position is a candidate iff logp[b, u] < below, compared on the recorded fp32 value (logp == 0 never qualifies at below == 0);
 *   2. candidates are ranked by (logp[b, u], u) ascending -- least likely first, ties by position -- and the first
 *      R_b = min(R, candidates) are chosen;
 *   3. base = the smallest multiple of K that is >= T_now[b] (= s when the steps are run in sequence).  For j < R_b:
 *      order[b, base + j] = the slot of rank j; the guide's entries of position base + j = those of position u; tokens[b, slot] = 22.
 *      Then T_now[b] = base + R_b, rounds_done[b] += 1, round_start[b, r] = base, round_count[b, r] = R_b.  A round with R_b == 0 is
 *      counted and appends nothing (every later round of that row is then empty too: its record does not change);
 *   4. positions in [old T_now[b], base) exist only when K > 1: their order becomes -1 ("holes").  They are never drawn (the step is
 *      already base) and their logp and dist entries keep their initial zeros.
 * Everything keyed by order position keeps that key: the Philox counter word of the draw, q_noise[t, row, :], logp[b, t], dist[b, t, :],
 * and generated dropout masks, keyed by the forward's first position.  Under the confident policy the selection permutes
 * [min(s, T_now), T_now) as it always does, so the appended positions are filled surest first.  The row's final token at a slot is the
 * one written at its live position; logp at earlier positions of that slot remains as history.  All of it runs on the device inside the
 * captured step (one launch in front of the forward); nothing is read back; a session repeats bit for bit.
 *
 * Capacity: the caller's Tmax must hold the worst case.  With e = T[b], repeat `rounds` times e = ceil(e / K) * K + R; the begin requires
 * e <= Tmax for every row, otherwise HD_ERR_INVALID (the message names the Tmax needed).  No buffer changes shape; hd_sample_run(t0, t1)
 * keeps taking order positions up to Tmax, and hd_sample runs up to the largest e.
 *
 * The same result can be had by chaining sessions from the host: for a round, a given-order session on the re-masked tokens whose order
 * holds the chosen slots at [base, base + R_b), run over those positions, draws the same tokens and records the same logp and dist bit
 * for bit (same K, noise key, guide, dropout mode).
 *
 * Lifetime: as the block size -- one-shot: the NEXT hd_sample_begin / hd_sample consumes it whether it succeeds or fails;
 * hd_sample_restart and the guards' repeats keep it and put T, order, the guide's entries and the counters back; hd_forward neither uses
 * nor clears it.  hd_set_refine: rounds == 0 clears; a NULL handle, rounds outside [0, 16], slots outside [1, 64], or a below that is
 * NaN, infinite or > 0 -> HD_ERR_INVALID (the values are looked at before the handle); inside an open session -> HD_ERR_STATE.  At the begin: a beam width, a confidence threshold, a
 * mutation budget, HD_DROPOUT_INJECT, or hd_score_begin / hd_score -> HD_ERR_UNSUPPORTED; a row whose order[b, 0:T[b]] repeats a slot
 * (a slot has ONE live position), or a Tmax below the capacity -> HD_ERR_INVALID.
 *
 * hd_refine_state copies T_now [B], round_start [B, rounds] (-1 for a round not opened) and round_count [B, rounds] out (each pointer
 * may be NULL), rows in whole-batch order whatever the lane split.  Legal where hd_sample_order is; a session without refinement ->
 * HD_ERR_STATE. */
HdStatus hd_set_refine(HdModel* m, int32_t rounds, int32_t slots, float below);   /* rounds == 0 clears */
HdStatus hd_refine_state(HdModel* m, int32_t* T_now /* [B] */, int32_t* round_start /* [B, rounds] */, int32_t* round_count /* [B, rounds] */);

/* ---- measurement helpers ------------------------------------------------------------------------
 * hd_sample_run brackets the steps it enqueues with HIP events on the handle's stream;
 * hd_last_run_ms returns the elapsed device time of the last completed run (after hd_sync/hd_sample_end); `steps` = t1 - t0 order
 * positions, which took ceil(steps / K) denoiser forwards in a session with K slots per step ("block decoding"). */
HdStatus hd_last_run_ms(HdModel* m, float* ms, int32_t* steps);
/* Algorithmic FLOPs of one forward of one row (SURVEY.md §8d formula). */
double hd_flops_per_row_forward(const HdConfig* cfg);
/* FLOPs one hd_sample step actually executes per row (last attention block pruned to the visited row, its value side
 * taken through the input rows instead of a V projection of every row). */
double hd_flops_per_row_sample_step(const HdConfig* cfg);
/* ---- precision routes --------------------------------------------------------------------------------
 * The reference computes in fp32 (PyTorch CPU / CUDA defaults, model/encoder/model.py:366-384).  gfx950 multiplies fp32 operands
 * on the matrix cores at 1/16 of the fp16 rate and has no TF32-like mode, so the library has three routes through the same
 * kernels' interfaces; all three hold the 1e-4 logit bound and reproduce the reference's recorded sampling traces bit for bit
 * (tests/test_prod_trace.py, tests/test_gpu_adversarial.py):
 *   HD_PRECISION_SPLIT     every large GEMM and the attention core as THREE fp16 MFMAs per fp32 product: each operand is hi + lo with
 *                          hi = fp16(x), lo = fp16(x - hi) (22 significand bits; x - hi is exact), a w ~= a_hi w_hi + a_hi w_lo +
 *                          a_lo w_hi with fp32 accumulation -- as close to the exact dot product as the fp32 kernels.  Launches of
 *                          fewer than 128 activation rows (none of the two models' single sequences), the pruned tail's compact GEMMs and the
 *                          static branch run the fp32 kernels.
 *   HD_PRECISION_F32_GEMM  GEMMs on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32); only the attention core (QK^T, PV) of launches
 *                          >= 8192 rows as three fp16 MFMAs per product (the round-3 default)
 *   HD_PRECISION_F32_ALL   every product on the fp32 MFMA pipe (rounds 1-2)
 *   HD_PRECISION_DEFAULT   what a handle starts with: the library default, HD_PRECISION_SPLIT since round 4 -- unless the environment
 *                          of hd_finalize overrides the DEFAULT (only the default; an explicit hd_set_precision wins):
 *                          HUDIFF_PRECISION=split|f32_gemm|f32_all, or the older switches HUDIFF_X3=0|1 (GEMMs) and
 *                          HUDIFF_ATTN_X3=0|1 (attention core).
 * hd_set_precision must be called before hd_finalize (the split weight images are built there); afterwards HD_ERR_STATE.
 *
 * Guards of the split kernels -- never an error, never a silently wrong row; the CALL is repeated inside the library and the event
 * is counted:
 *   range guard   split operands are not scaled, so the split is valid for |x| < 65504 only.  Every producer of a split checks
 *                 its values; when one is out of range, hd_forward / hd_sample[_end] repeats the whole call on the fp32 kernels (same
 *                 resident inputs, same noise key, same steps) and the handle stays on them (weights whose stream leaves the
 *                 range do so at every step) until hd_precision_reset.  hd_sample_restart and hd_sync notice the flag as well.
 *   weight guard  a split weight image scales its whole matrix by ONE power of two (largest |w| into [2^13, 2^14)), so entries far
 *                 below the largest one keep fewer than 22 bits (subnormal lo, then subnormal hi).  hd_finalize builds an image only
 *                 if every entry's (hi, lo) pair is within 2^-22 of the entry or, where that is larger, of the median |w| of the
 *                 matrix's NON-ZERO entries (a pruned matrix is judged by the entries it has) -- a property of the matrix alone,
 *                 true whenever its largest entry is within about 2^16 of that median.  A matrix that fails keeps its whole family
 *                 (ByteNet stacks / attention blocks) on the fp32 GEMMs; the other family keeps its images.  The report then reads:
 *                 split_built bit 0 clear (an image was refused, whichever family), lnsync_in_use 0 if the ByteNet family was
 *                 refused, split_built bit 1 unchanged (the core is built; a refused attention family runs attn_k beside its fp32
 *                 GEMMs, like split_layer_mask = 1), split_in_use unchanged (nothing was switched off by the range guard).
 *   ln_sync guard the ByteNet GEMMs of the split route normalise their own output rows: the N tiles of an M tile exchange LayerNorm
 *                 partials at a counter (write-through stores, agent-scope loads: correct wherever the blocks run), which presumes
 *                 they are co-resident.  A meeting that times out raises a flag; the call is repeated with separate LayerNorm passes
 *                 (ln_apply_k) and the handle keeps those.                                                                          */
enum { HD_PRECISION_DEFAULT = 0, HD_PRECISION_F32_GEMM = 1, HD_PRECISION_F32_ALL = 2, HD_PRECISION_SPLIT = 3 };
HdStatus hd_set_precision(HdModel* m, int32_t precision);
typedef struct HdPrecisionInfo {
    int32_t precision;          /* resolved route of the handle: HD_PRECISION_SPLIT / F32_GEMM / F32_ALL (never DEFAULT after hd_finalize) */
    int32_t split_built;        /* bit 0: split-precision weight images exist (GEMMs; none refused by the weight guard), bit 1: split-precision attention core */
    int32_t split_in_use;       /* 1 while eligible launches take the split kernels, 0 after the range guard switched them off   */
    int32_t lnsync_in_use;      /* 1 while the split ByteNet GEMMs normalise their own outputs, 0 = separate ln_apply_k passes   */
    int64_t range_fallbacks;    /* calls repeated on the fp32 kernels by the range guard                                          */
    int64_t lnsync_fallbacks;   /* calls repeated with ln_apply_k passes because an ln_sync meeting failed                        */
    int32_t last_call_repeated; /* 1 if the last hd_forward / hd_sample_end repeated its call (hd_last_run_ms then times the repeat) */
    int32_t lnsync_cross_xcd;   /* 1 once an ln_sync meeting saw its blocks on two XCDs: still correct (write-through hand-over), slower */
} HdPrecisionInfo;
/* size = sizeof(HdPrecisionInfo) of the caller (fields beyond it are not written) */
HdStatus hd_precision_report(HdModel* m, HdPrecisionInfo* out, size_t size);
/* The three original fields of the report (kept for round-3 callers). */
HdStatus hd_precision_info(HdModel* m, int32_t* split_built, int32_t* split_in_use, int64_t* range_fallbacks);
/* Puts a handle whose guards switched kernels off back on its configured route (between calls; HD_ERR_STATE inside a session). */
HdStatus hd_precision_reset(HdModel* m);
/* ---- tuning options ----------------------------------------------------------------------------------
 * The knobs that SELECT KERNELS or change how a batch is scheduled are part of the ABI (round 5; rounds 1-4 read them from the
 * environment only).  Every option has a library default (the value the published numbers use).  Precedence, as for the precision
 * route: an explicit hd_set_option wins; an option nobody set takes the environment variable named beside it if that is exported
 * when hd_create runs, else the default.  hd_set_option is legal between calls (HD_ERR_STATE inside a sampling session; options
 * marked [create] only before hd_finalize); it drops the handle's captured graphs.  Values outside [lo, hi] -> HD_ERR_INVALID.
 * None of them changes results beyond the last-ulp reassociation documented in INTEGRATION.md (tile shapes share one K order):
 * tests/test_gpu_x3.py test_tuning_options_interface (tokens) and tests/test_gpu_variants.py (every selectable kernel, stage by stage,
 * against a float64 evaluation; hd_debug_launch_tally below witnesses which kernel ran).                                          */
typedef enum HdOption {
    HD_OPT_LANES = 0,               /* HUDIFF_LANES            2     [1, 4]   lanes (stream + workspace + graph) a sampling batch is split into          */
    HD_OPT_LANE_MIN_ROWS = 1,       /* HUDIFF_LANE_MIN_B       16    [2, ..]  fewest rows of a batch that is split into lanes                           */
    HD_OPT_SPLIT_MIN_ROWS = 2,      /* HUDIFF_X3_ROWS          128   [1, ..]  fewest activation rows of a launch that takes the split-precision kernels   */
    HD_OPT_BIG_MIN_ROWS = 3,        /* HUDIFF_BIG_ROWS         8192  [1, ..]  fewest activation rows of a launch that takes the fp32 128-row-tile kernels */
    HD_OPT_LNSYNC_LEVEL = 4,        /* HUDIFF_X3_LNSYNC        2     [0, 2]   split ByteNet GEMMs normalise their own output: 0 no (ln_apply_k passes),
                                                                             1 the two inner GEMMs of a block, 2 the block's last GEMM as well           */
    HD_OPT_TAIL_FORM = 5,           /* HUDIFF_TAIL             2     {0, 2}   pruned tail of a sampling step: 0 twelve separate launches, 2 five sliced ones */
    HD_OPT_TAIL_MAX_ROWS = 6,       /* HUDIFF_TAIL_MAX_B       64    [0, ..]  largest lane that takes the sliced tail                                    */
    HD_OPT_SMALL_GRID = 7,          /* HUDIFF_X3_SMALL_GRID    320   [0, ..]  largest 128 x 128 grid of a split GEMM that takes 64 x 128 tiles instead    */
    HD_OPT_TINY_GRID = 8,           /* HUDIFF_X3_TINY_GRID     150   [0, ..]  largest 64 x 128 grid that takes 32 x 128 tiles instead                    */
    HD_OPT_LOADER_WAVES = 9,        /* HUDIFF_X3_LOADERS       1     [0, 1]   32 x 128 blocks carry four DMA-issuing waves while they fit one per CU      */
    HD_OPT_TINY_STAGES = 10,        /* HUDIFF_X3_TINY_NS       3     [2, 3]   LDS stages of the 32 x 128 split tiles                                     */
    HD_OPT_SMALL_STAGES = 11,       /* HUDIFF_X3_SMALL_NS      0     {0,2,3}  LDS stages of the 64 x 128 split tiles; 0 = three up to the grid below      */
    HD_OPT_SMALL_STAGES3_MAX_GRID = 12, /* HUDIFF_X3_SMALL_NS3_MAX 256 [0, ..]                                                                           */
    HD_OPT_ATTN_QSPLIT_MAX_GRID = 13,   /* HUDIFF_ATTN_QSPLIT_MAX 128 [0, ..] largest (sequence, head) grid whose query tiles are shared by two workgroups */
    HD_OPT_ATTN_WAVES = 14,         /* HUDIFF_ATTN_WAVES       12    {8, 12}  waves of the split attention core for L in (288, 304]                       */
    HD_OPT_LOOP_GRAPH = 15,         /* HUDIFF_LOOP_GRAPH       0     [0, 1]   1 = every hd_sample_run behaves as if HD_LOOP_GRAPH were set                 */
    HD_OPT_PRUNE_VALUE_VIA_ROWS = 16,   /* HUDIFF_PRUNE_V      1     [0, 1]   pruned last block: value side through the input rows (no V projection)      */
    HD_OPT_SPLIT_TILE = 17,         /* HUDIFF_X3_TILE          0     {0,128,256,512} force the big split GEMM tile: 128 x 128 / 256 x 128 / 256 x 256; 0 = by shape */
    HD_OPT_GEMM_SMALL_TILES = 18,   /* HUDIFF_GEMM_SMALL       1536  [0, ..]  fp32 launches with fewer 128-row tiles take 64 x 128 tiles                  */
    HD_OPT_STORE_NT = 19,           /* HUDIFF_ST_NT            0     [0, 1]   non-temporal epilogue stores in the fp32 GEMMs (the split GEMMs always use them) */
    HD_OPT_SPLIT_LAYER_MASK = 20,   /* HUDIFF_X3_MASK          3     [0, 3]   [create] bit 0 ByteNet blocks, bit 1 attention blocks get split weight images */
    HD_OPT_SPLIT_ATTN = 21,         /* HUDIFF_X3_ATTN          1     [0, 1]   split route: 0 keeps the fp32 attention core                                */
    HD_OPT_FUSED_ATTN = 22,         /* HUDIFF_FUSED_ATTN       1     [0, 1]   split route: the Q|K|V projection runs inside the attention kernel (one workgroup per
                                                                             (sequence, head group), K / V never leave the CU); 0 = projection GEMM + attention core    */
    HD_OPT_FUSED_ATTN_MIN_GRID = 23,/* HUDIFF_FUSED_ATTN_MIN_GRID 128 [0, ..] fewest (sequence, head group) workgroups -- over all lanes -- for which the fused
                                                                             form is taken (below, the two-launch form's finer tiles fill the chip better)        */
    HD_OPT_BN_CHAIN = 24,           /* HUDIFF_BN_CHAIN         0     [0, 3]   [create] split route: ByteNet stacks on the row-owner chain kernel (a wave owns whole rows
                                                                           through conv -> LN -> PFF3 -> residual -> LN -> PFF1 -> LN; n + 1 launches per stack): bit 0
                                                                           Dual / NanoConv, bit 1 token encoder; 0 (default: measured no faster, NOTES.md E) = three
                                                                           gemm_x3_k launches per block                                                                        */
    HD_OPT_BN_CHAIN_MIN_TILES = 25, /* HUDIFF_BN_CHAIN_MIN_TILES 128 [0, ..]  fewest workgroup tiles (128 rows; token encoder 256), over all lanes, that take the chain kernel */
    HD_OPT_COUNT = 26
} HdOption;
HdStatus hd_set_option(HdModel* m, int32_t option, int64_t value);
HdStatus hd_get_option(HdModel* m, int32_t option, int64_t* value);

/* Device facts for the bench JSON. */
HdStatus hd_device_info(int device, char* name, size_t name_len, int32_t* cu_count, int64_t* hbm_bytes);

/* ---- debugging aids (tests only) -----------------------------------------------------------------
 * hd_debug_stop_after: make hd_forward return after a stage (0 = off, 1 = token encoder, 2+n = before
 * attention block n, 100+n = right behind the first attention of block n); hd_debug_read copies an activation
 * buffer ("X","FEAT","Y","POS","EXTRA","AT","O","QKV"; split route also "ATX","YX") of the last call back as fp32
 * [B, L, width].  "AT" is x + A1(x) behind a block's first attention and at + A2(LN1(at)) behind its second on every
 * route: the split route keeps the second sum in split form only and the call decodes it (hi + lo); "O", "ATX",
 * "YX" are decoded the same way when the split kernels wrote them. */
HdStatus hd_debug_stop_after(HdModel* m, int32_t stage);
/* Makes the ln_sync meetings of the next call give up after one poll, so that the ln_sync guard (see "precision routes") fires and
 * its repeat path can be tested; cleared when the guard has fired. */
HdStatus hd_debug_fail_next_lnsync(HdModel* m);
HdStatus hd_debug_read(HdModel* m, const char* name, int32_t B, float* out, int64_t n_floats);
/* on != 0: the ln_sync launches deal the N tiles of an M tile to DIFFERENT XCDs (consecutive workgroup ids) instead of one XCD's
 * consecutive slots, so that the cross-XCD path of the meeting (write-through partials, agent-scope loads) is the one that runs;
 * results must be bit-identical to the normal placement and hd_precision_report then says lnsync_cross_xcd = 1. */
HdStatus hd_debug_scatter_lnsync(HdModel* m, int32_t on);
/* Launch tally: which kernels the handle's launchers chose since the last call of this function.  Counted on the HOST where the launch
 * is issued (no device code takes part), so a launch issued under graph capture counts once however often the graph is replayed, and a
 * handle that reuses a captured graph counts nothing: the witness is "> 0", never an exact number.  Copies min(n, HD_DBG_COUNT) counters
 * into `counts` (may be NULL with n = 0) and clears all of them.  The split GEMM ids come in pairs: id + 1 is the tap (conv) instantiation. */
typedef enum HdDebugKernel {
    HD_DBG_X3_256X256_S2 = 0,         /* gemm_x3_k: 256 x 256 tile, two stages (8 waves)                              */
    HD_DBG_X3_256X256_S2_CONV = 1,
    HD_DBG_X3_256X128_S3 = 2,         /*            256 x 128, three stages (8 waves)                                 */
    HD_DBG_X3_256X128_S3_CONV = 3,
    HD_DBG_X3_128X128_PLAIN = 4,      /*            128 x 128, plain epilogue set                                     */
    HD_DBG_X3_128X128_PLAIN_CONV = 5,
    HD_DBG_X3_128X128_LNSYNC = 6,     /*            128 x 128, ln_sync (meeting) epilogue set                         */
    HD_DBG_X3_128X128_LNSYNC_CONV = 7,
    HD_DBG_X3_64X128_S2 = 8,
    HD_DBG_X3_64X128_S2_CONV = 9,
    HD_DBG_X3_64X128_S3 = 10,
    HD_DBG_X3_64X128_S3_CONV = 11,
    HD_DBG_X3_32X128_S2 = 12,
    HD_DBG_X3_32X128_S2_CONV = 13,
    HD_DBG_X3_32X128_S3 = 14,
    HD_DBG_X3_32X128_S3_CONV = 15,
    HD_DBG_X3_32X128_S3_LOADERS = 16, /*            32 x 128, three stages, four DMA-issuing waves                    */
    HD_DBG_X3_32X128_S3_LOADERS_CONV = 17,
    HD_DBG_F32_128X128_BK16 = 18,     /* gemm_k (fp32 MFMA pipe)                                                      */
    HD_DBG_F32_128X128_BK32 = 19,
    HD_DBG_F32_64X128 = 20,
    HD_DBG_F32_32X128 = 21,
    HD_DBG_QKV_ATTN_19 = 22,          /* qkv_attn_x3_k<19, 1>: projection fused into the attention kernel             */
    HD_DBG_QKV_ATTN_10 = 23,          /* qkv_attn_x3_k<10, 2>                                                         */
    HD_DBG_ATTN_X3_19_W12 = 24,       /* attn_x3_k<19>, 12 waves                                                      */
    HD_DBG_ATTN_X3_19_W8 = 25,        /* attn_x3_k<19>, 8 waves                                                       */
    HD_DBG_ATTN_X3_10 = 26,           /* attn_x3_k<10>                                                                */
    HD_DBG_ATTN_F32 = 27,             /* attn_k (fp32 attention core)                                                 */
    HD_DBG_ATTN_QSPLIT = 28,          /* an attention core launch whose query tiles are shared by two workgroups      */
    HD_DBG_TAIL_SLICED = 29,          /* pruned tail: five sliced launches                                            */
    HD_DBG_TAIL_LAUNCHES = 30,        /* pruned tail: separate launches                                               */
    HD_DBG_VALUE_VIA_ROWS = 31,       /* pruned tail: value side through the input rows                               */
    HD_DBG_VALUE_VIA_PROJECTION = 32, /* pruned tail: value side through a V projection of every row                  */
    HD_DBG_SAMPLE_LANES_1 = 33,       /* hd_sample_run enqueued steps on 1 .. 4 lanes                                 */
    HD_DBG_SAMPLE_LANES_2 = 34,
    HD_DBG_SAMPLE_LANES_3 = 35,
    HD_DBG_SAMPLE_LANES_4 = 36,
    HD_DBG_LOOP_GRAPH = 37,           /* hd_sample_run launched the whole loop of a lane as one graph                 */
    HD_DBG_COUNT = 38
} HdDebugKernel;
HdStatus hd_debug_launch_tally(HdModel* m, int64_t* counts, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* HUDIFF_HIP_H */
