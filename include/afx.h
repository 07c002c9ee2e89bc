/*
 * afx.h -- C ABI of libafx.so, the MI355X (gfx950) native anti-spoof inference path.
 *
 * This is the drop-in boundary for the reference's model forward
 *   waveform (B,L) fp32  ->  logits (B,2) fp32   (index 1 = bonafide score)
 * i.e. what the reference obtains from `model(batch_x)` at main.py:210 and
 * trainer.py:106, for the model families of models/xlsr_aasist.py:5-177,
 * models/conformer_baseline.py:31-99 and the bare SSL extractor of
 * models/fe.py:8-40,53-99 / models/models.py:13-41.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer that is documented "device" is a
 *     HIP device pointer on the current device; `stream` is a hipStream_t passed as
 *     void* (NULL = the default stream).  Calls are asynchronous on that stream.
 *   - every function returns 0 on success, non-zero on error; afx_last_error() gives
 *     a thread-local message (mirrors the Python exceptions of the reference:
 *     ValueError text for bad layer counts etc.).
 *   - the caller owns inputs, outputs and the workspace; the handle owns only the
 *     packed weights.  A handle is re-entrant across streams as long as each
 *     concurrent call has its own workspace.
 *
 * The Python host side (real-time-deepfake-speech-detection_amd/afx/_lib.py) binds
 * exactly these symbols with ctypes; INTEGRATION.md shows the stub.
 */
#ifndef AFX_H_
#define AFX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct afx_engine* afx_handle;

enum { AFX_ARCH_SSL = 0, AFX_ARCH_XLSR_AASIST = 1, AFX_ARCH_CONFORMER = 2,
       AFX_ARCH_CONFORMER_HEAD = 3 /* MyConformer alone (models/conformer_baseline.py:8-29): class token, Conformer blocks, fc5; no trunk */ };
enum { AFX_EXTRACTOR_LAYER_NORM = 0, /* XLS-R: every conv layer conv+bias -> LayerNorm(512) -> GELU (what the reference loads) */
       AFX_EXTRACTOR_GROUP_NORM = 1  /* wav2vec2-base: bias-free convs, GroupNorm(512,512) on layer 0 only, GELU */ };
enum { AFX_DT_BF16 = 0, AFX_DT_FP16 = 1, AFX_DT_FP32 = 2, /* operand type (FP32: exact mode, fp32 MFMA); accumulation is always fp32 */
       AFX_DT_FP16X3 = 3 /* split precision: activations, LayerNorms, attention in fp32 as in exact mode; every dense product on
                            the fp16 matrix pipe as xh.wh + xl.wh + xh.wl (fp16 hi / lo pairs of both operands, ~22 significant
                            bits): the unconditional-parity mode at ~1/3 of the fp16 rate instead of 1/16 */ };

typedef struct afx_config {
  int arch;          /* AFX_ARCH_* */
  int dtype;         /* AFX_DT_* */
  int n_layers;      /* transformer layers in the SSL trunk, 1..24 (models/fe.py:60-62) */
  int conf_emb;      /* Conformer: emb_size   (models/conformer_baseline.py:38) */
  int conf_heads;    /*            heads      (:39) */
  int conf_kernel;   /*            kernel_size(:40) */
  int conf_blocks;   /*            n_encoders (:41) */
  int pre_emphasis;  /* 1: apply data/preprocess.py:16-29 inside the first kernel */
  float pre_emphasis_coef;
  int extractor_mode; /* AFX_EXTRACTOR_* (fairseq extractor_mode "layer_norm" / "default"); checkpoint keys
                         feature_extractor.conv_layers.0.2.{weight,bias} instead of ....{i}.2.1.* and no conv biases */
} afx_config;

/* ---- lifecycle ---------------------------------------------------------------- */
int afx_create(const afx_config* cfg, afx_handle* out);
void afx_destroy(afx_handle h);
const char* afx_last_error(void);
const char* afx_version(void);   /* "afx <ver> (gfx950) build <id> hip <toolchain version>" */
const char* afx_build_id(void);  /* hash of the sources the library was built from (tools stamp profiles/ with it) */
/* HIP_VERSION the library was compiled with / the runtime this process resolved (hipRuntimeGetVersion); afx/_lib.py refuses a
 * different major version (no reference counterpart: the reference has no native code) */
int afx_hip_versions(int* build, int* runtime);

/* ---- weights: reference checkpoint key names, without
 * the optional "module." prefix (utils.py:13-43).  `dev_ptr` is a contiguous fp32
 * device tensor; it is copied / repacked, the caller may free it afterwards.
 * Unknown-but-harmless keys (quantizer.*, project_q.*, final_proj.*, mask_emb,
 * *.bn1.*, num_batches_tracked) return 0 and are ignored. ------------------------- */
int afx_load_weight(afx_handle h, const char* name, const float* dev_ptr, const int64_t* shape, int ndim,
                    void* stream);
/* fold BatchNorms / weight-norm, check that every required tensor arrived */
int afx_finalize(afx_handle h, void* stream);

/* ---- forward ------------------------------------------------------------------ */
int afx_num_frames(int n_samples);                       /* T after the 7 conv layers */
size_t afx_workspace_bytes(afx_handle h, int B, int L);  /* scratch needed by one call */
/* wave: device (B,L) fp32.  logits: device (B,2) fp32.  L is free (test_duration_sec, config.py:75): at least
 * 400 samples (one SSL frame); the AASIST head needs >= 6 frames and holds at most 629 temporal graph nodes
 * (T <= 1889 SSL frames, clips up to about 37 s); beyond either bound the call fails with a message, it never truncates. */
int afx_forward(afx_handle h, const float* wave, int B, int L, float* logits, void* ws, size_t ws_bytes,
                void* stream);
/* The same forward in two calls, for scoring loops that overlap the back-end of one batch with the trunk of the next
 * (main.py:199-221 scores batch after batch; nothing orders batch i's head before batch i+1's trunk but the one stream):
 * afx_trunk_forward(ws) on stream A leaves the SSL features inside `ws`; afx_head_from_workspace(ws) on stream B -- after an
 * event the caller records behind the trunk -- runs the back-end on them.  Two workspaces alternate; a workspace is reused
 * for a trunk only after its head has finished.  Same kernels, same results as afx_forward, bit for bit. */
int afx_trunk_forward(afx_handle h, const float* wave, int B, int L, void* ws, size_t ws_bytes, void* stream);
int afx_head_from_workspace(afx_handle h, int B, int L, float* logits, void* ws, size_t ws_bytes, void* stream);
/* SSL features only: feats device (B,T,1024) fp32 == extract_feat() of models/fe.py:17-21 */
int afx_ssl_forward(afx_handle h, const float* wave, int B, int L, float* feats, void* ws, size_t ws_bytes,
                    void* stream);
/* Ragged batches (clips of different lengths in one call; the length policy of data/test_set.py:201-248 is what makes
 * the reference's batches uniform -- un-cropped clips are the case it leaves to batch size 1).  wave: device (B,Lmax) fp32,
 * row b holds clip b's n_samples[b] samples followed by ZEROS; n_samples: HOST int[B].  Each clip is scored exactly as if it
 * were alone: key-padding masks in both attentions, zero padding past its own frames in the positional / depthwise convs,
 * per-length sub-batches for the AASIST graphs.  logits (B,2).  Synchronises the stream once (length upload). */
size_t afx_ragged_workspace_bytes(afx_handle h, int B, int Lmax);
int afx_forward_ragged(afx_handle h, const float* wave, int B, int Lmax, const int* n_samples, float* logits, void* ws,
                       size_t ws_bytes, void* stream);
/* feats device (B,Tmax,1024) fp32 with Tmax = afx_num_frames(Lmax), rows past a clip's own frames zeroed;
 * n_frames (HOST int[B], may be NULL) receives the frame counts */
int afx_ssl_forward_ragged(afx_handle h, const float* wave, int B, int Lmax, const int* n_samples, float* feats,
                           int* n_frames, void* ws, size_t ws_bytes, void* stream);
/* The path from the OUTPUT OF CONV LAYER 5 on: conv5_h device (B,T5,512) in the operand type (fp16 / bf16; fp32 in exact
 * mode) -> conv layer 6, feature LayerNorm, projection, positional conv, transformer layers, head -> logits (B,2).
 * Same kernels in the same order as afx_forward from that point, so a caller that keeps conv layers 0-5 incrementally
 * (they are causal-local: a new 250-ms chunk adds 800/400/200/100/50/25 frames, the rest of the 4-s window is unchanged)
 * reproduces afx_forward(window) bit for bit at a sixteenth of the conv cost (afx/streaming.py, BASELINE config 5). */
size_t afx_tail_workspace_bytes(afx_handle h, int B, int T5);
int afx_tail_forward(afx_handle h, const void* conv5_h, int B, int T5, float* logits, void* ws, size_t ws_bytes,
                     void* stream);
/* the same with the window inside a longer per-stream buffer: utterance b's T5 rows start at conv5_h + b * batch_stride
 * elements (0 = packed; a multiple of 8, at least T5 * 512) -- a streaming caller appends the new frames to a ring and
 * passes a view, no copy per hop */
int afx_tail_forward_strided(afx_handle h, const void* conv5_h, long batch_stride, int B, int T5, float* logits, void* ws,
                             size_t ws_bytes, void* stream);
/* the same over B windows at arbitrary offsets of ONE layer-5 buffer (an offline timeline: the conv stack runs once over a
 * whole recording, afx/timeline.py): window b is the T5 rows that start at element offs[b] of conv5_h, which holds
 * total_elems elements.  Windows may overlap and may come from different recordings sharing the buffer.  offs: HOST
 * long long[B], each a multiple of 8 with offs[b] + T5 * 512 <= total_elems -- checked before anything is launched.  A
 * gather kernel packs the windows into the workspace (their offsets travel as kernel arguments: no upload, asynchronous),
 * then the packed tail runs: window b's logits equal afx_tail_forward's on those rows copied contiguous, bit for bit. */
size_t afx_tail_windows_workspace_bytes(afx_handle h, int B, int T5);
int afx_tail_forward_windows(afx_handle h, const void* conv5_h, long long total_elems, const long long* offs, int B, int T5,
                             float* logits, void* ws, size_t ws_bytes, void* stream);
/* ---- KV-cached streaming mode (BASELINE config 5 as named: "250 ms chunks with cached SSL-encoder KV state") ----------
 * NOT A REFERENCE FUNCTION: the reference's trunk is bidirectional over the clip, an encoder that sees every frame once
 * -- when its chunk arrives -- is a different model (block-causal: a chunk's frames attend to the chunk and to the cached
 * keys / values of the 15 chunks before it, the positional conv sees no frame beyond the chunk).  Parity target: the
 * build's own offline restatement oracle/streaming.py.  An afx_kv holds the per-stream state of
 * n_streams lock-stepped streams (K / V rings of every layer, the positional conv's left context, the feature window);
 * afx_kv_step consumes the NEW frames of conv layer 6 of every stream, (n_streams, n, 512) fp32 with 1 <= n <= 16, and
 * returns the back-end's logits on the window that ends with this chunk.  The handle must outlive its afx_kv objects; weights
 * reloaded into the handle do not refresh keys / values already cached.
 * Layout of the state (what a host-side model of it may assume; oracle/insitu_kv.py does): per layer and stream a ring of
 * 256 [q | k | v] rows (3072 operand-type elements) in 16 groups of 16 slots, stream s's slot i at ring row 256 s + i.  The
 * chunk of step number `hop` (counted from afx_kv_create, every lock-step and ragged step adds one) is written to group
 * hop % 16 of every stream, frame r at slot 16 group + r; the group then holds as many live slots as the chunk brought
 * frames (a shorter chunk leaves the previous occupant's rows in the slots past its count: written earlier, never live).
 * The positional conv's left context is the stream's newest 64 projected rows in the operand type (zeros before its
 * first chunk); the feature window is a 208-row fp32 buffer per stream, right-aligned, zeros above the frames it has, of
 * which the back-end scores the newest min(frames, 200). */
typedef struct afx_kv afx_kv;
int afx_kv_create(afx_handle h, int n_streams, afx_kv** out);
void afx_kv_destroy(afx_kv* kv);
size_t afx_kv_state_bytes(const afx_kv* kv);
size_t afx_kv_workspace_bytes(const afx_kv* kv, int n_frames);
int afx_kv_step(afx_kv* kv, const float* feats6, int n_frames, float* logits, void* ws, size_t ws_bytes, void* stream);
/* Per-stream sessions: every stream still brings one chunk per step, but streams start at different steps.
 * afx_kv_reset makes the listed slots (distinct, 0 <= slot < n_streams) begin a new stream with the next step: their
 * cached keys / values, positional-conv context and feature window are dropped.  afx_kv_step_ragged takes the chunks as
 * (n_streams, n_max, 512) fp32 with stream b's n_frames[b] (host array, 1 <= n_frames[b] <= n_max <= 16) frames first;
 * each stream's logits equal, bit for bit, those of the same stream stepped from its reset in a fresh afx_kv.  Once
 * either is called, the state is per stream and afx_kv_step refuses it.  A reset stream's base group (the group of its
 * first chunk, from which its 16 groups are visited in order) is the group the next step writes, hop % 16; its 16 valid
 * counts, its left context and its window start empty.  A block's rows past its own n_frames[b] are computed and written
 * to their slots but never live, and they are zero in the positional conv's operand. */
int afx_kv_reset(afx_kv* kv, const int* slots, int n_slots, void* stream);
size_t afx_kv_ragged_workspace_bytes(const afx_kv* kv, int n_max);
int afx_kv_step_ragged(afx_kv* kv, const float* feats6, int n_max, const int* n_frames, float* logits, void* ws, size_t ws_bytes,
                       void* stream);
/* Non-paced streams: a step over a list of active streams.  slots: host, n_active distinct stream indices
 * (0 <= slot < n_streams) in any order; feats6: device (n_active, n_max, 512) fp32, row i = the chunk of slots[i] with its
 * n_frames[i] (host array, 1 <= n_frames[i] <= n_max <= 16) new frames first; logits: device (n_active, 2) in list order.
 * Only the listed streams advance: every other stream's cached keys / values, positional-conv context, feature window and
 * ring position stay as they are.  Each stream writes its chunks at its own ring group (its base group plus its own step
 * count), so a stream's logits equal, bit for bit, those of the same stream stepped on every step of a fresh afx_kv.
 * n_active == 0 launches nothing.  The workspace is carved for n_active streams (afx_kv_active_workspace_bytes).  The
 * first call makes the state per stream; afx_kv_step and afx_kv_step_ragged then refuse it (afx_kv_reset still applies:
 * a reset stream starts at its own next group, which becomes its base group).  At the first call every stream's next
 * group is the group a lock-step or ragged step would have written, hop % 16; from then on a listed stream writes its
 * own next group and moves it on by one (mod 16), and the step count `hop` stands still. */
size_t afx_kv_active_workspace_bytes(const afx_kv* kv, int n_active, int n_max);
int afx_kv_step_active(afx_kv* kv, const int* slots, int n_active, const float* feats6, int n_max, const int* n_frames,
                       float* logits, void* ws, size_t ws_bytes, void* stream);
/* Moving sessions: a stream's state leaves one afx_kv and takes over a slot of another (another size, another GPU, the
 * same afx_kv, after host memory).  afx_kv_export copies the listed streams (host slots, distinct, 0 <= slot < n_streams)
 * into payload (device, 16-byte aligned, n x afx_kv_slot_bytes bytes: the k and v thirds of the stream's ring rows in
 * every layer, 16 groups x 16 rows in the stream's own order from its first group on; the positional conv's 64-frame
 * context; the 208-row feature window) and writes one host meta row of AFX_KV_META ints per stream: [0] the layout word
 * (layers, dtype, element size, ring / context / window rows, format), [1] the stream's next group relative to its first,
 * [2] its window length, [3] 0, ints [4, 8) its 16 valid counts as bytes in the payload's group order.  The state is read
 * only: no byte of it changes and a lock-stepped state stays lock-stepped.  One stream synchronisation per call.
 * afx_kv_import makes the listed slots of kv take over those streams (their own are dropped; the other slots keep every
 * byte): it refuses a meta row whose layout word differs from kv's, or that is out of range, before anything changes.
 * The imported stream's next chunk lands where kv writes next and its keys are visited in the order they had, so each
 * stream's logits continue, bit for bit, as in the afx_kv it left.  The first import makes kv per stream (afx_kv_step then
 * refuses it, as after afx_kv_reset).  n == 0 launches nothing. */
#define AFX_KV_META 8
size_t afx_kv_slot_bytes(const afx_kv* kv);
int afx_kv_export(afx_kv* kv, const int* slots, int n, void* payload, int* meta, void* stream);
int afx_kv_import(afx_kv* kv, const int* slots, int n, const void* payload, const int* meta, void* stream);
/* back-end alone from given SSL features (B,T,1024) fp32 -> logits (B,2) */
int afx_head_forward(afx_handle h, const float* feats, int B, int T, float* logits, void* ws, size_t ws_bytes,
                     void* stream);
size_t afx_head_workspace_bytes(afx_handle h, int B, int T);
/* MyConformer.forward (models/conformer_baseline.py:22-29) alone: tokens device (B,T,emb) fp32 (what Model.forward hands it
 * after LL / BatchNorm / SELU, :58-63) -> class token prepended, the n_encoders Conformer blocks -> logits (B,2) = fc5(token 0)
 * and, when `embedding` is not NULL, token 0 itself (B,emb).  Handles of arch CONFORMER or CONFORMER_HEAD; workspace
 * afx_head_workspace_bytes(h, B, T). */
int afx_conformer_forward(afx_handle h, const float* tokens, int B, int T, float* logits, float* embedding, void* ws,
                          size_t ws_bytes, void* stream);
/* Overflow guard (no reference counterpart: the reference computes in fp32, models/fe.py:11-21).  The half-precision
 * engines keep operand copies in fp16 / bf16 (fp16x3: fp16 hi / lo pairs); a checkpoint with outlier channels can push one
 * past the format's range, after which the scores are NaN -- or, behind the AASIST head's max-pooling and top-k, finite
 * garbage.  Every forward counts, on the device and for free, the rows of the trunk's final LayerNorm whose statistics are
 * not finite and the logits that are not finite; this call waits for `stream`, returns non-zero (afx_last_error names the
 * counts and the precision) when anything was counted since the last check, and clears the counters.  A scoring loop calls
 * it once before it writes its scores (afx/harness.py does). */
int afx_check_finite(afx_handle h, void* stream);
/* debug taps (off by default; when on, forward keeps fp32 copies of intermediates) */
int afx_enable_taps(afx_handle h, int on);
/* debug taps: copy an intermediate of the LAST forward on this workspace into `out`
 * (device fp32).  Names: "conv", "proj", "pos", "layer<N>", "ssl", "tokens",
 * "block<N>", "e_S", "e_T", "hidden".  Returns the element count through n_out. */
int afx_tap(afx_handle h, const char* name, float* out, size_t cap_elems, size_t* n_out, void* stream);

/* ---- per-kernel-class timing (hipEvents on the launch stream around every launch of
 * the forwards issued between begin and end; off otherwise).  afx_profile_end waits
 * for the recorded events and returns, per class, summed milliseconds, algorithmic
 * FLOPs and launch counts (arrays of afx_profile_num_classes() entries). ------------ */
int afx_profile_begin(afx_handle h);
int afx_profile_end(afx_handle h, int n_classes, double* ms, double* flops, long long* launches);
int afx_profile_num_classes(void);
const char* afx_profile_class_name(int cls);

/* per-handle switches between two forms of the same op (A/B measurements and the per-op reference paths of the tests):
 * "posconv_sliding" 1 (default) sliding-window positional conv / 0 chunked-K GEMM; "conf_attn_mfma" 1 matrix-core Shaw
 * attention / 0 the fp32 VALU kernel; "fuse_conformer" 1 fused row chains / 0 one kernel per op; "fuse_conv_ln" 1 conv +
 * LayerNorm + GELU in one kernel / 0 two.  They act on THIS handle only. */
int afx_engine_set(afx_handle h, const char* key, int value);
/* "concurrent" (afx_engine_set, default 0): 1 says that the native calls which follow run beside another forward on a second
 * stream (Engine.forward_lanes / forward_overlapped set it around their calls and clear it after).  Launch shapes are then
 * chosen for CU time (workgroups x unit: what a launch keeps from the other forward) instead of makespan (rounds x unit: the
 * launch alone on the chip) -- taller GEMM tiles, 8 waves per workgroup in the fused Conformer chains.  Same rows, bit for
 * bit.  afx_engine_get reads "concurrent" back and "objective": what the last native call on the handle ran under. */
int afx_engine_get(afx_handle h, const char* key, int* value);
/* The launch plan of a half- or split-precision product, host arithmetic only (no device, no handle).  rpb / kchunk: 0 = M / K
 * (a plain product).  flags: 1 fused LayerNorm epilogue (N = 512), 2 split precision, 4 an activation outside the lean
 * epilogue, 8 never the deep 128x64 tile.  objective: 0 makespan, 1 CU time, -1 what a launch outside any forward gets (the
 * forced "dispatch_objective" knob when it is set, else makespan; no call leaves an objective behind).  out[8]: tile family,
 * instance, tile rows, tile slots, rows of the first launch when split (else 0), the remainder's instance, its tile slots,
 * the objective used.  afx_conf_chain_waves: waves per workgroup of a fused Conformer chain over M token rows. */
int afx_gemm_plan(int M, int N, int K, int rpb, int kchunk, int groups, int flags, int objective, int* out);
int afx_conf_chain_waves(int M, int objective);
/* tuning knobs for A/B measurements (process-wide; not part of the drop-in surface).
 * "gemm_map": workgroup->tile order of the MFMA GEMM, -1 default, 0 linear, 1 XCD-
 * contiguous, 2 XCD-contiguous + grouped.  "gemm_tile": -1 auto, 0 128x128, 1 256x256.
 * "fuse_conv_ln": 1 (default) conv layers 1-6 use the fused LayerNorm epilogue, 0 two kernels.
 * "aasist_conv_slots": 0 automatic, n > 0 caps the grid of the AASIST back-end's persistent conv kernel at n workgroups
 * (a test knob: a small problem then walks many tiles per workgroup).
 * "dispatch_objective": -1 per call (default), 0 / 1 every launch by makespan / CU time.  "dispatch_cu_mask": which decisions
 * the CU-time objective takes over (1 height of the 256-wide tile, 2 chain waves, 4 height of the conv tile, 8 the two row
 * splits; default 3: the two that won their A/B).  "conf_chain_waves": 0 by the objective, 4 / 8 forced.
 * None of these changes WHAT is computed; the timing-only switches that do ("gemm_nodma") exist only in the
 * attribution build (make attr), the product library refuses them. */
int afx_debug_set(const char* key, int value);

/* ---- single-kernel entry points (unit parity tests; operand pointers are bf16 or
 * fp16 device arrays according to `dtype`; fp32 arrays for AFX_DT_FP32 and, in afx_k_gemm / afx_k_mhsa, for
 * AFX_DT_FP16X3: the split-precision forms take and return fp32 -- afx_k_gemm then builds the hi / lo operand forms
 * per call in temporary device memory and synchronises: a test hook) --------------------------------------------- */
/* out = resid + alpha act(A W^T + bias): A (M, K) with row stride lda, W (N, K) with row stride ldw, resid / out_f fp32 (M, N)
 * with row strides ldr / ldo_f, out_h operand type (fp32 for the fp32 operand types) with row stride ldo_h; strides count
 * elements.  Shapes: M >= 1, N % 4 == 0, K % 64 == 0 (fp32: K % 16 == 0; fp16x3: K % 32 == 0 and packed rows, lda == ldw
 * == K).  Alignment: the kernels read 16 bytes of an operand row at a time and read and write fp32 rows 16 bytes at a
 * time, so every row must START on a 16-byte boundary: A, W, bias, resid, out_f 16-byte aligned, lda % 8 == 0 and ldw % 8 ==
 * 0 for the half types (% 4 for fp32), ldr % 4 == 0, ldo_f % 4 == 0.  out_h is written 8 halfs at a time where N % 8 == 0
 * (out_h 16-byte aligned, ldo_h % 8 == 0) and 4 at a time otherwise (8-byte aligned, ldo_h % 4 == 0); as fp32: 16-byte
 * aligned, ldo_h % 4 == 0.  Nothing is read past column K of a row, past row M - 1 of A / resid or row N - 1 of W, and
 * nothing is written outside the M x N elements of an output.  A violation of the shape or alignment rules: non-zero,
 * afx_last_error names `gemm`, nothing launched. */
int afx_k_gemm(int dtype, const void* A, long lda, const void* W, long ldw, int M, int N, int K, const float* bias,
               int act, float alpha, const float* resid, long ldr, float* out_f, long ldo_f, void* out_h, long ldo_h,
               void* stream);
/* Conv1d(Cin->N, k, stride s) on channel-last input (B,Tin,Cin) as one GEMM; Wp is
 * the tap-major packed weight [N][k*Cin]; out_f (B,Tout,N) fp32 */
int afx_k_conv_gemm(int dtype, const void* in_h, const void* Wp, int B, int Tin, int Tout, int Cin, int k, int s,
                    int N, const float* bias, float* out_f, void* stream);
/* the same conv with LayerNorm over the 512 output channels + activation fused into the GEMM
 * epilogue (row-complete tile); N is fixed at 512; out_f and/or out_h (B,Tout,512) */
int afx_k_conv_ln_act(int dtype, const void* in_h, const void* Wp, int B, int Tin, int Tout, int Cin, int k, int s,
                      const float* bias, const float* gamma, const float* beta, float eps, int act, float* out_f,
                      void* out_h, void* stream);
int afx_k_pack_linear(int dtype, const float* w, int N, int K, int Kpad, void* out_h, void* stream);
int afx_k_pack_conv(int dtype, const float* w, int N, int Cin, int k, void* out_h, void* stream);
int afx_k_conv0(int dtype, const float* wave, int B, int L, const float* w, const float* bias, const float* gamma,
                const float* beta, int pre_emph, float coef, void* out_h, void* stream);
/* the same without the per-call operand build of the test hook above (device allocation + stream synchronisation): the
 * layer's split-precision fp16 operand block is built once per checkpoint into afx_k_conv0_pack_bytes() bytes and passed in;
 * asynchronous, allocates nothing -- what the streaming scorer runs every hop */
size_t afx_k_conv0_pack_bytes(void);
int afx_k_conv0_pack(const float* w, const float* bias, void* pack, void* stream);
int afx_k_conv0_packed(int dtype, const float* wave, int B, int L, const void* pack, const float* w, const float* bias,
                       const float* gamma, const float* beta, int pre_emph, float coef, void* out_h, void* stream);
/* data/preprocess.py:16-29 as a stand-alone op: y[t] = x[t] - coef*x[t-1], reflect pad */
int afx_k_pre_emphasis(const float* x, int B, int L, float coef, float* y, void* stream);
/* Utterance length policy, batched (data/test_set.py:139-146 pad, :201-227 adjustDuration, :229-248
 * adjustDuration_random_start): x = the ragged clips packed back to back (device), offs[B+1] their sample
 * offsets (device, int64), starts[B] crop starts or NULL; out (B, duration): out[b][i] = x_b[(start_b + i) mod n_b]. */
int afx_k_tile_crop(const float* x, const long long* offs, const long long* starts, int B, int duration, float* out,
                    void* stream);
/* Polyphase resampling of an integer input rate r to 16 kHz (afx/resample.py builds the taps): g = gcd(16000, r),
 * L = 16000/g up, M = r/g down, h = firwin(2*half_len + 1, 1/max(L, M), window=("kaiser", 5.0)) * L with
 * half_len = 10*max(L, M) (scipy.signal.resample_poly's default design, float64); taps (L, T) fp32 with
 * taps[p][j] = h[p + j*L] (0 past the end), T = ceil(len(h)/L).  Causal, zero history before the first sample:
 *     y[n] = sum_{j<T} taps[p][j] * x[i0 - j],  i0 = floor(n*M/L),  p = n*M mod L,  x[<0] = 0
 * = upfirdn(h, x, L, M)[:ceil(N*L/M)], fp32 with one fma chain per output in ascending j; it lags resample_poly by
 * half_len/M output samples.  Offline: x = clips packed back to back (device), in_offs / out_offs[B+1] their input and
 * output offsets (device, int64; out_offs[b+1] - out_offs[b] = ceil(n_b*L/M)), max_out = the longest output row.
 * M/L <= 12. */
int afx_k_resample(const float* x, const long long* in_offs, const long long* out_offs, int B, long long max_out,
                   const float* taps, int L, int M, int T, float* out, void* stream);
/* The same function streamed: row i of x (A, n_in) is the next chunk of the stream in slot slot[i] (int32, device,
 * distinct); it is resampled as hist[slot[i]] ++ x[i] (hist (S, T-1) fp32: the stream's last T-1 samples, zeros for a
 * new stream) into exactly n_in*L/M outputs (n_in*L % M == 0), then hist[slot[i]] takes the last T-1 samples of that
 * concatenation.  Each output gets the offline form's inputs, taps and order: chunked output is bit-identical to the
 * whole stream resampled by afx_k_resample.  Rows of slots not named are untouched. */
int afx_k_resample_stream(const float* x, int A, int n_in, float* hist, const int* slot, const float* taps, int L, int M,
                          int T, float* out, void* stream);
/* Packet ingest (afx/ingest.py): bytes as a service receives them -> each slot's 16 kHz pending ring, in one launch for
 * all packets of a feed.  stage (device, stage_bytes): the encoded payloads; hdr (device, rows x 8 int32), per row:
 *     slot, byte offset of the row's first sample in stage (a multiple of the sample size), n_in samples, n_out outputs,
 *     p0 = n_done*M mod L, d0 = floor(n_done*M/L) - N, wpos (where the ring takes the first output), 0
 * for a slot that had received N input samples and made n_done = ceil(N*L/M) outputs; n_out = ceil((N+n_in)*L/M) - n_done
 * (the host reduces these from its int64 counters; slots of one call are distinct).  encoding 0 pcm_f32le, 1 pcm_s16le
 * (v / 32768), 2 G.711 mu-law, 3 G.711 A-law (ITU-T G.711 to the 16-bit linear value, / 32768): exact in fp32.  Output k
 * of a row is output n_done + k of afx_k_resample over the slot's whole decoded stream,
 *     y = sum_{j<T} taps[p][j] * v[i - j],  i = d0 + floor((k*M + p0)/L),  p = (k*M + p0) mod L,
 * v = the decoded packet, and hist[slot] (S, T-1: the stream's T-1 samples before the packet, zeros for a new stream)
 * at negative positions -- the same inputs, fp32 taps and ascending-j fma chain, so the bits do not depend on where the
 * stream was cut.  It is written to ring[slot][(wpos + k) mod ring_len] (ring (S, ring_len) fp32; max_out = the largest
 * n_out <= ring_len), then hist[slot] takes the last T-1 samples of hist[slot] ++ the decoded packet (rows with n_out = 0
 * included).  taps NULL with L = M = T = 1: the identity, sample k decoded into the ring, no history.  A row whose header
 * would leave stage, hist or ring is skipped whole.  M/L <= 12, T - 1 <= 256. */
int afx_k_ingest(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_out, int encoding,
                 const float* taps, int L, int M, int T, float* hist, float* ring, int S, int ring_len, void* stream);
/* afx_k_ingest over rows of different formats (afx/ingest.py MixedPacketScorer): a format is (encoding, taps, L, M, T), taps
 * NULL with L = M = T = 1 the identity, as above.  formats (HOST, n_formats entries, 1..16) is read during the call and travels
 * to the kernel by value: there is no device table; taps are device pointers.  hdr rows are afx_k_ingest's with the eighth int
 * = the row's format index; a row is validated against ITS format (index in range, p0 < L, offset a multiple of its sample
 * size, payload inside stage, and afx_k_ingest's other checks) and skipped whole when it fails.  Output k of a row has the
 * value afx_k_ingest gives it in a launch of that one format: the same decoder, inputs, taps and ascending-j fma chain.
 * max_out (HOST, n_formats ints): per format the largest n_out among its rows of this call, 0 = no row of it (its rows, if
 * any, then write no output).  hist (S, Hs) fp32, Hs >= every format's T - 1: a slot of format f carries its T_f - 1 samples
 * in the first columns of its row, which one further launch over all rows advances (identity rows are skipped); hist may be
 * NULL when every format is the identity.  Refused with nothing launched: n_formats outside 1..16, a bad encoding, a bad
 * filter shape, T - 1 > 256, M/L above 12, a null stage / hdr / ring, a max_out beyond ring_len, Hs below a format's T - 1. */
typedef struct afx_ingest_format {
  const float* taps; /* device, (L, T) fp32; NULL: the identity */
  int encoding, L, M, T;
} afx_ingest_format;
int afx_k_ingest_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, const afx_ingest_format* formats,
                       int n_formats, const int* max_out, float* hist, int Hs, float* ring, int S, int ring_len, void* stream);
/* out (A, hop) fp32: out[i][k] = ring[slot_i][(head_i + k) mod ring_len], table (device, A x 2 int32) = (slot_i, head_i):
 * the next hop of the named slots as the streaming scorers' push takes it.  The ring is only read. */
int afx_k_ingest_pop(const float* ring, int S, int ring_len, const int* table, int A, int hop, float* out, void* stream);
/* Payload expand (afx/codecs.py): the verb that runs before ingest / place.  The kernels above and below read a payload by
 * random access; a payload they cannot index that way is first written as fp32 samples into another zone of the same staging
 * buffer and read from there as encoding 0 (pcm_f32le).  stage (device, stage_bytes) is read AND written; hdr (device,
 * rows x 4 int32), per row:
 *     source byte offset in stage, source bytes B, destination byte offset in stage (a multiple of 4), codec number
 * The row's n samples go to ((float*)(stage + destination))[0..n); the rows of one launch write disjoint ranges that no row
 * reads.  Codec numbers, every decode exact in fp32:
 *     0 dvi4       RFC 3551 4.5.1 (IMA ADPCM), the payload is ONE block: predict (int16, big-endian), index (uint8), one
 *                  reserved byte, then 4-bit codes, the high nibble of each byte first; n = 2 (B - 4).  The header is the state
 *                  before the first code.  Per code c, with the standard 89-entry step table and the index table
 *                  (-1, -1, -1, -1, 2, 4, 6, 8) twice:
 *                      step = STEP[index];  index = clamp(index + IDX[c], 0, 88)
 *                      d = (step >> 3) + (c & 4 ? step : 0) + (c & 2 ? step >> 1 : 0) + (c & 1 ? step >> 2 : 0)
 *                      pred = clamp(c & 8 ? pred - d : pred + d, -32768, 32767);  sample = pred / 32768
 *     1 pcm_s16be  big-endian int16, v / 32768; n = B / 2
 *     2 pcm_s24be  big-endian 24-bit two's complement, v / 8388608; n = B / 3
 *     3 pcm_u8     offset-128 bytes, (b - 128) / 128; n = B
 * One wave per DVI4 block: 64 codes a step, both recurrences as prefix scans over clamp-add maps, (pred, index) carried from
 * step to step; the PCM codecs are a map.  max_n = the largest n of the launch.  A row is skipped whole, writing nothing, when
 * its codec number is outside 0..3, its source splits a sample, it is a DVI4 block under 4 bytes or with header index > 88, or
 * its source or destination leaves stage.  Refused with nothing launched, each with a message naming the entry point: a null
 * stage / hdr, rows outside 1..65535, a max_n below 0 or beyond what stage can hold (4 max_n > stage_bytes). */
int afx_k_payload_expand(void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, void* stream);
/* Jitter buffer (afx/jitter.py): per slot one DECODED reorder ring, jring (S, J) fp32; input-rate sample i of the slot's
 * played-out stream E (indexed from the session's first accepted timestamp) lives at column i mod J.  All indices are the
 * host's (playout point, received intervals, gaps); nothing is read back.  With lookback = max(T-1, P+F) the host keeps every
 * launch of a round that has released E below `cur` inside the J consecutive indices [cur - lookback, cur + J - lookback).
 * Each of the three verbs (place, conceal, release) is one kernel over a table of rates (afx_k_jitter_*_rates below); the four
 * entry points here are its case of one rate, built from their scalar arguments: one table entry, Js = J, rows without a rate
 * index.  What they write and what they refuse is stated here.
 * afx_k_jitter_place: one launch for all packet sub-ranges of a feed.  hdr (device, rows x 4 int32), per row: slot, byte
 *     offset of the sub-range's first sample in stage (a multiple of the sample size), n samples, ring column c of the
 *     first: jring[slot][(c + k) mod J] = decode(sample k), k < n, with afx_k_ingest's encodings and exact decode.  The rows
 *     of one launch write disjoint ranges (the host splits packets at the playout point and at what was received before).
 *     max_n = the largest n <= J.  A row whose header would leave stage or jring is skipped whole. */
int afx_k_jitter_place(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, int encoding,
                       float* jring, int S, int J, void* stream);
/* afx_k_jitter_place_mixed: afx_k_jitter_place with the encoding read per row.  hdr (device, rows x 5 int32), per row: slot,
 *     byte offset (a multiple of the row's sample size), n, ring column c, encoding (0..3 as for afx_k_ingest).  The ring is
 *     decoded, so rows of different encodings may follow each other in one slot's stream.  A row with an encoding outside 0..3
 *     is skipped whole, like one that would leave stage or jring. */
int afx_k_jitter_place_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, float* jring, int S,
                             int J, void* stream);
/* afx_k_jitter_conceal: a released gap of E that began at index a is written into the ring.  hdr (device, rows x 4 int32),
 *     per row: slot, a mod J, d_lo, d_hi: for d in [d_lo, d_hi), E[a + d] = jring[slot][(a + d) mod J] =
 *         mode 0 (zero):    0
 *         mode 1 (repeat):  fade[d] * E[a - P + (d mod P)] for d < F, 0 for d >= F
 *     one fp32 multiply of two stored fp32 values; fade (device, F fp32), P the repeat period, F the fade length.  The
 *     source [a - P, a) is read from the ring as it stands (it may hold an earlier gap's concealed samples): gaps of one
 *     slot go in successive launches, the rows of one launch are of distinct slots.  max_n = the largest d_hi - d_lo; a row
 *     needs d_hi + P <= J (source and written columns disjoint), else it is skipped whole; max_n + P > J is refused. */
int afx_k_jitter_conceal(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* fade, int P, int F,
                         int mode, void* stream);
/* afx_k_jitter_release: afx_k_ingest with the ring as its input.  hdr (device, rows x 8 int32), per row: slot, a0 mod J,
 *     n_in, n_out, p0, d0, wpos, 0 for a slot whose playout point a0 = N moves to N + n_in (p0, d0, n_out reduced from N as
 *     for afx_k_ingest).  Output k of a row is output ceil(N*L/M) + k of afx_k_resample over all of E:
 *         y = sum_{j<T} taps[p][j] * v[i - j],  i = d0 + floor((k*M + p0)/L),  p = (k*M + p0) mod L,
 *     v[k] = jring[slot][(a0 + k) mod J] for k >= -(T-1) (the filter history is the ring's own earlier columns; zeros
 *     after a reset) -- the same inputs, fp32 taps and ascending-j fma chain -- written to ring[slot][(wpos + k) mod
 *     ring_len], the pending 16 kHz ring afx_k_ingest_pop reads.  taps NULL with L = M = T = 1: a copy.  Slots of one launch
 *     are distinct; max_out = the largest n_out <= ring_len; n_in <= J, T - 1 <= J, M/L <= 12.  A row whose header would
 *     leave a ring, or with n_out > max_out, is skipped whole: it writes nothing.  The eighth int is not read. */
int afx_k_jitter_release(const float* jring, int S, int J, const int* hdr, int rows, int max_out, const float* taps, int L,
                         int M, int T, float* ring, int ring_len, void* stream);
/* The jitter buffer over slots of different clock rates (afx/jitter.py MixedJitterScorer).  A rate is (taps, L, M, T) as for
 * afx_k_jitter_release (taps NULL with L = M = T = 1: the identity), its ring length J = lookback + W with
 * lookback = max(T-1, P+F), its repeat period P and fade length F in that rate's samples and its fade table (device, max(F, 1)
 * fp32; read in mode 1 only).  rates (HOST, n_rates entries, 1..16) is read during the call and travels to the kernels by
 * value: there is no device table; taps and fade are device pointers.  jring is (S, Js) fp32 with Js >= every rate's J: a slot
 * at rate f keeps sample i of its stream at column i mod J_f of its row, uses the columns [0, J_f) only and never touches a
 * column at or beyond J_f, so the sizing invariant above holds per slot with its own J_f.  A row names its rate by an index, the
 * last int of its header, and is validated against ITS rate (index in range, column < J_f, n <= J_f, d_hi + P_f <= J_f,
 * p0 < L_f, and the other checks stated above); a row that fails writes nothing.  Every value written is the one the
 * one-rate entry point writes in a launch of that rate: it is the same kernel, so the same decoder, the same single fp32
 * multiply, the same inputs, taps and ascending-j fma chain.
 * afx_k_jitter_place_rates: hdr (device, rows x 6 int32): afx_k_jitter_place_mixed's five ints, then the rate index;
 *     jring[slot][(c + k) mod J_f] = decode(sample k), k < n.  max_n = the largest n.
 * afx_k_jitter_conceal_rates: hdr (device, rows x 5 int32): afx_k_jitter_conceal's four ints, then the rate index; the
 *     function of afx_k_jitter_conceal with the row's P_f, F_f, fade_f and J_f.  mode (0 zero, 1 repeat) is the launch's; in
 *     mode 0 the rates' P, F and fade are not read (P_f = 0 below).  max_n = the largest d_hi - d_lo.
 *     For both, max_n is refused when NO rate of the table can hold such a row, max_n + P_f > J_f for every f (place: P_f = 0):
 *     with one rate that is max_n > J, or max_n + P > J; with several it refuses only launches whose largest row every rate
 *     would skip on the device anyway.
 * afx_k_jitter_release_rates: hdr (device, rows x 8 int32): afx_k_jitter_release's, the eighth int the rate index.  max_out
 *     (HOST, n_rates ints): per rate the largest n_out among its rows of this call, 0 = no row of it (a row with more outputs than its
 *     rate's max_out writes nothing).  The grid and the dynamic LDS are the largest over the rates present; a workgroup beyond its row's
 *     outputs leaves before it stages anything.
 * Refused with nothing launched: n_rates outside 1..16, a null table, a bad filter shape, T - 1 > J, J outside 1..Js, M/L
 * above 12, mode 1 with a null fade or P <= 0, a null stage / hdr / jring / ring / max_out, rows outside 1..65535, a max_n no
 * rate can hold, a max_out beyond ring_len.  Each refusal names its entry point; the one-rate entry points refuse the same. */
typedef struct afx_jitter_rate {
  const float* taps; /* device, (L, T) fp32; NULL: the identity */
  const float* fade; /* device, (max(F, 1),) fp32: fp32(1 - d/F); may be NULL in mode 0 */
  int L, M, T, J, P, F;
} afx_jitter_rate;
int afx_k_jitter_place_rates(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n,
                             const afx_jitter_rate* rates, int n_rates, float* jring, int S, int Js, void* stream);
int afx_k_jitter_conceal_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const afx_jitter_rate* rates,
                               int n_rates, int mode, void* stream);
int afx_k_jitter_release_rates(const float* jring, int S, int Js, const int* hdr, int rows, const afx_jitter_rate* rates,
                               int n_rates, const int* max_out, float* ring, int ring_len, void* stream);
/* Comfort noise (afx/jitter.py ComfortNoise; RFC 3389 silence in a DTX call): the fourth verb of the jitter buffer.  The host
 * splits a released gap at its governing silence marks; the parts after a mark are noise, written into the ring like concealed
 * samples.  The value of index i (64 bits, from the session's origin) at level l (0..127, -dBov) with the launch's seed, all
 * integer arithmetic mod 2^32:
 *         x = lo32(i) * 0x9E3779B9 + hi32(i) * 0x85EBCA6B + seed
 *         x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *         k = int32(x) >> 8                  (arithmetic shift: -2^23 <= k < 2^23, exactly an fp32 number)
 *         E[i] = amp[l] * fp32(k)            (one correctly rounded fp32 multiply)
 *     amp (device, 128 fp32): amp[l] = fp32(sqrt(3) * 10^(-l/20) / 2^23), computed in float64 and rounded once: uniform white
 *     noise of RMS 10^(-l/20) of the decoders' full scale.  The value depends on (seed, i, l) only; nothing is clipped.
 * afx_k_jitter_noise: hdr (device, rows x 6 int32), per row: slot, ring column c of the first index i0, n, lo32(i0), hi32(i0),
 *     level: jring[slot][(c + k) mod J] = amp[level] * fp32(k(seed, i0 + k)), k < n.  The rows of one launch write disjoint
 *     ranges; a slot may have several (noise has no source, so there are no ranks).  max_n = the largest n <= J.  A row is
 *     skipped whole, writing nothing, when its slot is outside [0, S), c outside [0, J), n outside [0, J], level outside
 *     0..127 or hi32(i0) < 0.
 * afx_k_jitter_noise_rates: hdr (device, rows x 7 int32): the six ints, then the rate index; the same function with the row's
 *     J_f; a row with a rate index out of range is skipped whole.  Of a rate only J is read.
 * Refused with nothing launched, as for the other verbs: a null jring / hdr / amp, rows outside 1..65535, a max_n no rate can
 * hold, and for _rates what afx_k_jitter_place_rates refuses of a table.  Each refusal names its entry point. */
int afx_k_jitter_noise(float* jring, int S, int J, const int* hdr, int rows, int max_n, unsigned seed, const float* amp,
                       void* stream);
int afx_k_jitter_noise_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const afx_jitter_rate* rates,
                             int n_rates, unsigned seed, const float* amp, void* stream);
/* Pitch-period concealment (afx/jitter.py conceal="pitch_sync"): a released gap repeats the last PITCH PERIOD of E, found by an
 * exact integer search, under a hold and a fade.  afx_k_jitter_conceal and its mode argument are unchanged (mode 2 stays
 * refused); these are two verbs of their own.  Lengths in the slot's input-rate samples: lags Pmin..Pmax, correlation window
 * Wc, fallback period P0 in [Pmin, Pmax], hold Hd, fade F, G = Hd + F, history Lh = Pmax + Wc.  For a gap with origin a, d = i - a:
 *         q[j]  = quant(E[j]) for j in [a - Lh, a);  E[<0] = 0 (the ring's zeros after a reset)
 *         quant(x): y = x * 32768f (one fp32 multiply);  NaN -> 0;  else clamp(rint(y) (ties to even), -32768, 32767), an integer
 *         for p in Pmin..Pmax:
 *             c(p) = sum_{j in [a-Wc, a)} q[j] * q[j-p]           (exact integers: any summation order gives the same number)
 *             e(p) = sum_{j in [a-Wc, a)} q[j-p]^2
 *             s(p) = (double(c) * double(c)) / double(e)  if c > 0 and e > 0, else no candidate
 *                    (one fp64 multiply and one fp64 divide, each correctly rounded)
 *         p* = the p with the largest s(p), the smallest such p on a tie;  P0 if there is no candidate
 *         E[a + d] = gain[d] * E[a - p* + (d mod p*)]  for d < G   (one fp32 multiply of two stored fp32 values);  0 for d >= G
 *         gain[d] = 1 for d < Hd;  fp32(1 - (d - Hd)/F) for Hd <= d < G    (computed in float64, rounded once)
 * afx_k_jitter_pitch: the estimate.  hdr (device, rows x 2 int32), per row: slot, a mod J, for the gaps whose origin is released
 *     now; rows of one launch are of distinct slots.  One workgroup per row writes p* to period[slot] (device, (S,) int32: state
 *     of the slot's open gap, never read back).  A row is skipped whole, writing nothing, when its slot is outside [0, S), its
 *     column outside [0, J) or Lh > J.
 * afx_k_jitter_conceal_period: the synthesis.  hdr as for afx_k_jitter_conceal (rows x 4 int32: slot, a mod J, d_lo, d_hi), gain
 *     (device, max(G, 1) fp32), p* read from period[slot]; a stored value outside [Pmin, Pmax] is read as P0, so a row never
 *     reads outside [a - Pmax, a).  max_n = the largest d_hi - d_lo; a row needs d_hi + Pmax <= J (source and written columns
 *     disjoint), else it is skipped whole.
 * The _rates forms: rows end in their rate index (3 and 5 int32); lags (HOST, n_rates entries) is parallel to rates and travels
 *     by value like it.  Of a rate J is read, and by the synthesis fade (its gain table, Hd_f + F_f entries) and F; a row with a
 *     rate index out of range, or Lh_f > J_f, is skipped whole.  The one-rate entry points are the table of one entry.
 * Refused with nothing launched, each refusal naming its entry point: a null jring / hdr / period / table (synthesis: gain), rows
 *     outside 1..65535, Pmin < 1, Pmax < Pmin, Wc < 1, P0 outside [Pmin, Pmax], a negative hold or fade, no rate whose ring holds
 *     Lh (estimate) or max_n + Pmax (synthesis), an Lh beyond 32000 samples (64 KB of LDS), and what afx_k_jitter_place_rates
 *     refuses of a table. */
typedef struct afx_jitter_lags {
  int Pmin, Pmax, Wc, P0, Hd;
} afx_jitter_lags;
int afx_k_jitter_pitch(const float* jring, int S, int J, const int* hdr, int rows, int Pmin, int Pmax, int Wc, int P0, int* period,
                       void* stream);
int afx_k_jitter_pitch_rates(const float* jring, int S, int Js, const int* hdr, int rows, const afx_jitter_rate* rates,
                             const afx_jitter_lags* lags, int n_rates, int* period, void* stream);
int afx_k_jitter_conceal_period(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* gain,
                                const int* period, int Pmin, int Pmax, int P0, int Hd, int F, void* stream);
int afx_k_jitter_conceal_period_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const afx_jitter_rate* rates,
                                      const afx_jitter_lags* lags, int n_rates, const int* period, void* stream);
/* Speech gate (afx/vad.py): an energy gate with noise-floor tracking and hangover over frames of `frame` 16 kHz samples
 * (160 = 10 ms), per slot.  Constants, fp32: e_floor (the mean-square floor times frame), ratio > 1, rise >= 1, and
 * nf_min = e_floor / ratio (one fp32 division); hang >= 0 frames.  State per slot: nf (S,) fp32, +inf for a new stream, and
 * h (S,) int32, 0 for a new stream.  The energy e of a frame x[0..frame) is a sum of squares in ONE order, every operation
 * a single correctly rounded fp32 multiply or add (no fma):
 *     sq[i] = x[i]*x[i];  p[l] = sq[l] + sq[l + 64] + sq[l + 128] + ... for l < 64, ascending, only indices < frame (a lane
 *     with none holds 0);  for w = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + w], l < w;  e = p[0]
 * Per frame, in stream order:
 *     speech = e < inf && e > max(e_floor, ratio * nf)           (nf = inf: not speech)
 *     if (e < inf) nf = max(nf_min, min(e, nf * rise))           (a non-finite e leaves nf alone)
 *     if (speech) h = hang;   keep = speech || h > 0;   if (!speech && h > 0) h -= 1
 * so exactly `hang` frames after the last speech frame are kept, and none before an onset.
 * afx_k_gate: x (A, n) fp32 on the device, n a positive multiple of frame; row i is the next n samples of the stream in
 * slot hdr[i][0] (hdr: device, A x 2 int32 = slot, wpos; the slots of one call are distinct).  The kept frames of row i
 * are copied bit for bit, in order, to ring[slot][(wpos + k) mod ring_len] (ring (S, ring_len) fp32, the layout
 * afx_k_ingest_pop reads); kept[i] (A,) int32 on the device receives the number of samples kept; nf[slot] and h[slot] take
 * the state after the row; mask, (A, n / frame) bytes on the device or NULL, receives every frame's keep flag (0 / 1).
 * Rows of slots not named are untouched.  A row whose header would leave the state or the ring (slot outside [0, S), wpos
 * outside [0, ring_len)), or whose n exceeds ring_len, is skipped whole with kept[i] = 0 (its mask row is not written).
 * One launch takes at most 512 frames of every row (its per-frame tables live in LDS); a longer row goes in successive
 * launches on the same stream that carry nf, h and kept through device memory: the result does not depend on the split. */
int afx_k_gate(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
               float* nf, int* h, float* ring, int S, int ring_len, int* kept, unsigned char* mask, void* stream);
/* Look-ahead gate (afx/vad.py LookaheadGate): onset pre-roll.  The decision per frame (energy order, speech, nf, h, keep)
 * is afx_k_gate's, unchanged.  On top of it a delay line of `pre` frames per slot (1 <= pre <= 31).  With G the index of a
 * frame in its stream since the reset (0, 1, ...), per frame, in stream order, after the decision above:
 *     if (speech)   every frame now in the line is flagged
 *     if (G >= pre) frame G - pre leaves the line; it is EMITTED iff its flag is set
 *     frame G enters the line with flag = keep
 * that is keep'[g] = keep[g] || any(speech[g+1 .. g+pre]): frame g is decided, and emitted if kept, while frame g + pre is
 * processed; the newest `pre` frames of a stream are always undecided (a hop of zeros decides them: a zero frame is never
 * speech and flags nothing).  The gated stream is the concatenation of the emitted frames, copied bit for bit.
 * afx_k_gate_la: x, n, frame, the constants, nf, h, ring, kept as for afx_k_gate; kept[i] = the samples EMITTED by row i.
 *     hdr (device, A x 4 int32) = slot, wpos, F, 0: F = the frames the slot was pushed since its reset (so row i holds
 *     frames F .. F + n/frame - 1); wpos and ring_len are whole frames.
 *     flags (S,) int32: bit (g mod pre) is the flag of delayed frame g; bits of blocks not yet filled are 0.
 *     line (S, pre * frame) fp32: delayed frame g at block g mod pre; the delayed frames are [max(0, F - pre), F).
 *     src (S, ring_len / frame) int32: entry w / frame = the index g of the frame emitted at ring position w.
 *     mask, (A, n / frame) bytes or NULL: entry j = keep' of frame F - pre + j, 0 where that is negative.
 * A new stream has F = 0 and flags = 0 (the line's contents are then never read).  A row with slot outside [0, S), wpos
 * outside [0, ring_len) or off the frame grid, n > ring_len, F < 0 or F + n/frame >= 2^31 is skipped whole with kept[i] = 0
 * and nothing else written.  Rows of slots not named are untouched.  ring_len a multiple of frame, at most 2^30.  Rows of
 * more than 512 frames go in successive launches that carry nf, h, flags, line and kept through device memory: the result
 * does not depend on the split.  Within a launch the frames that leave the line are copied out of it before any frame is
 * stored into it (frame G enters the block frame G - pre leaves). */
int afx_k_gate_la(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
                  int pre, float* nf, int* h, int* flags, float* line, float* ring, int* src, int S, int ring_len, int* kept,
                  unsigned char* mask, void* stream);
/* Tone gate (afx/vad.py ToneGate): the plain gate plus a per-frame Goertzel bank at K signalling frequencies (1 <= K <= 16;
 * DTMF, call progress, fax), so that a confirmed tone is not speech, is not kept and ends the hangover.  Constants, fp32,
 * each computed in float64 and rounded once on the host: coef[k] = 2 cos(2 pi f_k / 16000) (device, (K,) fp32) and
 * thr = frac * frame / 2 (a sinusoid of amplitude a over N samples has energy about a^2 N / 2 and Goertzel power about
 * a^2 N^2 / 4, so T >= thr * e reads "at least frac of the frame's energy sits at one or two bank frequencies");
 * confirm >= 1 and hold >= 0 frames.  State per slot: afx_k_gate's nf and h, and tone_state (S, 3) int32 = r (tonal frames
 * in a row), q (hold frames left), tones (tone frames since the reset); (0, 0, 0) for a new stream.  Every arithmetic
 * operation is a single correctly rounded fp32 multiply, add or subtract (no fma).  Per frame, in stream order:
 *     e, speech, the nf update: afx_k_gate's (same energy order, same operations)
 *     for every k:  s1 = s2 = +0.0
 *                   for i = 0 .. frame-1:  t = c_k * s1;  t = t - s2;  s0 = x[i] + t;  s2 = s1;  s1 = s0
 *                   a = s1 * s1;  b = s2 * s2;  m = c_k * s1;  m = m * s2;  P_k = (a + b) - m
 *     p1, p2 = the two largest of { P_k : P_k > +0.0 } as a multiset (a NaN or non-positive P_k counts as +0.0; fewer than
 *              two leave +0.0);  T = p1 + p2
 *     tonal = e < inf && e > e_floor && T >= thr * e             (one fp32 multiply; false for any NaN)
 *     r = tonal ? min(r + 1, 2^31 - 1) : 0;   if (r >= confirm) q = hold
 *     tone = r >= confirm || q > 0;   if (r < confirm && q > 0) q -= 1;   tones = min(tones + tone, 2^31 - 1)
 *     if (tone) { speech = false; h = 0; }
 *     if (speech) h = hang;   keep = speech || h > 0;   if (!speech && h > 0) h -= 1
 * so r >= confirm implies q == hold, and 0 <= q <= hold.  The first confirm - 1 frames of a burst are decided as afx_k_gate
 * decides them (there is no look-ahead); exactly `hold` frames after the last confirmed frame are still tone; a stream with
 * no tonal frame is gated exactly as afx_k_gate gates it.  The gated stream is the kept frames, copied bit for bit.
 * afx_k_gate_tone: x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept as for afx_k_gate.  Optional
 * outputs on the device, each may be NULL: ntone (A,) int32, the tone frames of each row; mask (A, n / frame) bytes, bit 0
 * keep, bit 1 tone, bit 2 tonal; tsum (A, n / frame) fp32, the T of every frame.  A row whose header would leave the state
 * or the ring, or whose n exceeds ring_len, is skipped whole: its state is untouched, kept[i] = 0 and ntone[i] = 0, its mask
 * and tsum rows are left as they were.  Rows of more than 512 frames go in successive launches that carry nf, h,
 * tone_state, kept and ntone through device memory: the result does not depend on the split.  A bad scalar argument (a
 * NULL among the required pointers, A outside 1..65535, n not whole frames, K outside 1..16, thr not finite or not > 0,
 * confirm < 1, hold < 0, or what afx_k_gate refuses) returns an error and launches nothing. */
int afx_k_gate_tone(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
                    const float* coef, int K, float thr, int confirm, int hold, float* nf, int* h, int* tone_state, float* ring,
                    int S, int ring_len, int* kept, int* ntone, unsigned char* mask, float* tsum, void* stream);
/* Talk spurts (afx/turns.py): a slot's stream cut into turns, each scored as one utterance.  A turn is a maximal run of
 * kept frames (bit 0 of a gate's mask, hangover frames included), cut when it reaches max_frames.  Two buffers per slot:
 * bufs (S, 2, max_frames * frame) fp32.  State per slot, all 0 for a new stream: state (S, 3) int32 = open (0 / 1: the buffer
 * that collects the open turn), n (its frames, 0 <= n < max_frames), g (the source index of its first frame); totals (S, 4)
 * int32 = scored, short, cut, kept, each saturating at 2^31 - 1.  A launch names rows i = 0..A-1 of distinct slots: hdr
 * (device, A x 3 int32) = slot, wpos, g0; row i holds the F frames g0 .. g0 + F - 1 of the slot's stream, mask (A, F) bytes
 * says which are kept, and the kept ones stand in order, frame after frame, at staging[slot][(wpos + k) mod ring_len]
 * (staging (S, ring_len) fp32: what a gate launch with ring = staging and that wpos wrote).  Per row, r = 0 and
 * done = (0, 0, 0, 0); for j = 0 .. F-1 with G = g0 + j:
 *     if (mask[j] & 1) {
 *         if (n == 0) g = G;
 *         bufs[slot][open][n * frame .. (n + 1) * frame) = staging frame r   (bit for bit);   r += 1; n += 1; kept += 1
 *         if (n == max_frames) { done = (open, n, g, G + 1); scored += 1; cut += 1; open ^= 1; n = 0; }
 *     } else if (n > 0) {
 *         if (n >= min_frames) { done = (open, n, g, G); scored += 1; open ^= 1; }
 *         else                 short += 1;
 *         n = 0;
 *     }
 * done (A, 4) int32 = buffer, frames, first source frame, one past the last, of the turn the row completed; (0, 0, 0, 0) when
 * it completed none.  With F <= min_frames a row completes at most one scored turn, so after the row the buffer that is not
 * `open` holds the completed turn or nothing of use: afx_k_turn_collect reads it before the slot's next row.  A turn shorter
 * than min_frames is dropped and counted; the remainder of a cut turn is a new turn.  The contents of a buffer beyond the
 * open turn's n frames (and beyond a completed turn's) are not defined: a dropped turn's frames need not be copied.
 * afx_k_turn: one workgroup of 256 threads per row; thread 0 runs the recurrence and writes a per-frame copy plan to LDS,
 * the four waves then copy a frame per wave and step, 16 bytes per lane where frame, ring_len and wpos are multiples of 4
 * and staging and bufs are 16-byte aligned, one sample per lane otherwise.  A row with slot outside [0, S), wpos outside
 * [0, ring_len), g0 < 0 or g0 + F >= 2^31 (or whose slot's state is no turn state: open not 0 / 1, n outside [0, max_frames))
 * is skipped whole: done[i] = (-1, -1, -1, -1) and nothing else is written.  Rows of slots not named are untouched.  Refused
 * with nothing launched: a NULL pointer, A outside 1..65535, F outside 1..512, frame <= 0, min_frames < F, min_frames >
 * max_frames, S <= 0, F * frame > ring_len, max_frames * frame > 2^30. */
int afx_k_turn(const float* staging, int S, int ring_len, const unsigned char* mask, const int* hdr, int A, int F, int frame,
               int min_frames, int max_frames, float* bufs, int* state, int* totals, int* done, void* stream);
/* The clip of a turn of L = frames * frame samples is the turn repeated to the window, clip[k] = turn[k mod L] for
 * k < max_frames * frame (afx_k_tile_crop's function with start 0; a cut turn is its own clip).
 * afx_k_turn_collect: rows (device, R x 3 int32) = slot, buffer, frames; out[r][k] = bufs[slot][buffer][k mod L], out
 * (R, max_frames * frame) fp32, copied bit for bit.  Grid over (column tiles, row); four samples per lane where frame is a
 * multiple of 4 and bufs and out are 16-byte aligned, one otherwise.  A row with slot outside [0, S), buffer outside 0..1 or
 * frames outside 1..max_frames is skipped whole (its output row is left as it was).  Refused with nothing launched: a NULL
 * pointer, S <= 0, R outside 1..65535, frame <= 0, max_frames <= 0, max_frames * frame > 2^30. */
int afx_k_turn_collect(const float* bufs, int S, int max_frames, int frame, const int* rows, int R, float* out, void* stream);
/* The close step of the recurrence: the end of a call.  Applied to a slot's (open, n, g) and totals:
 *     if (n >= min_frames) { done = (open, n, g, g + n); scored += 1; open ^= 1; }
 *     else if (n > 0)      { short += 1;                 done = (0, 0, 0, 0); }
 *     else                                               done = (0, 0, 0, 0);
 *     n = 0;
 * cut and kept do not move; the counters saturate at 2^31 - 1.  The closed turn stands in the buffer done names, for
 * afx_k_turn_collect, as after afx_k_turn.
 * afx_k_turn_close: slots (device, A int32) names A distinct slots of state (S, 3) and totals (S, 4); done (A, 4) int32.  One
 * thread per row.  A row whose slot is outside [0, S), or whose slot's state is no turn state (open not 0 / 1, n outside
 * [0, max_frames)), gets done = (-1, -1, -1, -1) and nothing else is written for it.  Refused with nothing launched: a NULL
 * pointer, A outside 1..65535, S <= 0, min_frames < 1, min_frames > max_frames. */
int afx_k_turn_close(const int* slots, int A, int S, int min_frames, int max_frames, int* state, int* totals, int* done,
                     void* stream);
/* Turns offline (afx.turns.score_turns): a whole stream cut at once.  The cut of a keep mask of n frames: the recurrence of
 * afx_k_turn from a new stream's state over frames 0 .. n-1 (no audio moves), then, with close_end, the close step.  The
 * scored turns are the done values with frames > 0, in stream order; each is (first, end) in source frames with two flags:
 * cut (bit 0: it closed by reaching max_frames) and at_end (bit 1: the close step closed it; its end is n).  Short turns are
 * counted, not listed.  Without close_end the turn still open behind frame n-1 is open = (first, frames), (-1, 0) when there
 * is none; with close_end open = (-1, 0).  A turn is a run of kept frames, so its samples are contiguous in the source.
 * afx_k_turn_scan: mask (device bytes, bit 0 = kept; the other bits are ignored) holds the frames of A recordings back to
 * back; offs (device, A + 1 int64, non-decreasing) their frame offsets: row i is mask[offs[i] .. offs[i+1]), fewer than 2^31
 * frames; a row of no frames is legal (a row whose offsets are negative, decrease or span 2^31 frames or more is taken as
 * one).  Per row the cut above.  Outputs, all device int32: row_base (A + 1), the exclusive prefix sums of the scored turns
 * per row, row_base[A] = their total R (sums clamp at 2^31 - 1); table (cap, 4) = row, first, end, flags, ordered by row,
 * then by first -- the order is the stream's, no atomic decides it; totals (A, 4) = scored, short, cut, kept; open (A, 2).
 * With R > cap the first cap table rows are written, nothing beyond them is touched, and row_base, totals and open are the
 * true ones.  One workgroup of 256 threads per row, 4096 frames a step (16 mask bytes per thread, one 16-byte load where
 * the 16 frames lie inside the row and on a 16-byte boundary of the address, byte loads at a row's two ends): a max-scan of
 * run starts and a sum-scan of scored turns over the workgroup per step, a carry from step to step; a count pass, one
 * workgroup over the A row counts, and a write pass (skipped when cap = 0), three launches on `stream`.  Refused with
 * nothing launched: a NULL pointer, A outside 1..65535, min_frames < 1, min_frames > max_frames, cap < 0. */
int afx_k_turn_scan(const unsigned char* mask, const long long* offs, int A, int min_frames, int max_frames, int close_end,
                    int* table, int cap, int* row_base, int* totals, int* open, void* stream);
/* afx_k_turn_clips: the clips of scored turns, tiled from the source.  x (device fp32) holds A recordings back to back, xoffs
 * (device, A + 1 int64) their sample offsets; for r < R, (row, first, end) = table[r0 + r][0..2], read on the device, and
 * out[r][k] = x[xoffs[row] + first * frame + (k mod L)], L = (end - first) * frame, k < max_frames * frame, copied bit for
 * bit; out (R, max_frames * frame) fp32.  Grid over (column tiles, row); four samples per lane where frame is a multiple of
 * 4 and out and the turn's first sample are 16-byte aligned, one otherwise.  A row with row outside [0, A), first < 0,
 * end <= first, end - first > max_frames, or end * frame beyond its recording (or xoffs[row] < 0) is skipped whole: its
 * output row is left as it was.  Refused with nothing launched: a NULL pointer, A < 1, r0 < 0, R outside 1..65535,
 * frame <= 0, max_frames <= 0, max_frames * frame > 2^30. */
int afx_k_turn_clips(const float* x, const long long* xoffs, int A, int frame, int max_frames, const int* table, int r0, int R,
                     float* out, void* stream);
/* Cascade (afx/cascade.py): a cheap screen scores every slot at every hop; the windows of the slots whose score looks
 * suspicious are gathered for a second model, under a per-push budget and a per-slot cooldown.  Every index comes from a
 * host-built header (device int32), nothing is allocated, all three run on `stream`.  State: hist (S, window) fp32, the
 * retained audio, sample t of a session at column t mod window; wait (S,) int32, 0 for a new stream.
 * The selection.  A push names rows i = 0..A-1: slot b_i (distinct), score s_i (fp32), elig_i.  With fp32 compares,
 *     cand_i       = elig_i && wait[b_i] == 0 && s_i < threshold      (a NaN score: never; threshold = +inf: every finite or -inf score)
 *     before(j, i) = s_j < s_i || (!(s_i < s_j) && b_j < b_i)         (ties, -0.0 / +0.0 included, go to the lower slot)
 *     rank_i       = the number of candidates j with before(j, i)
 *     chosen_i     = cand_i && rank_i < budget
 *     wait[b_i]    = chosen_i ? cooldown : max(wait[b_i] - 1, 0)      (named slots only)
 * There is no ageing: a candidate the budget passed over keeps wait == 0 and competes again at its next hop.
 * afx_k_cascade_store: x (A, hop) fp32; hdr (A x 2 int32) = slot, wpos: hist[slot][(wpos + k) mod window] = x[i][k], k < hop
 *     (hop <= window).  Four samples per lane where wpos, hop and window are multiples of 4 and both rows are 16-byte
 *     aligned, one per lane otherwise: any wpos in [0, window), any hop and window.  Rows of slots not named are untouched;
 *     a row with its slot outside [0, S) or its wpos outside [0, window) is skipped whole.
 * afx_k_cascade_select: scores (A,) fp32 on the device, s_i = scores[i * stride] (stride >= 1: a column of a logits matrix is
 *     read in place); hdr (A x 2 int32) = slot, elig (0 / non-zero); 1 <= A <= 8192 (one
 *     workgroup ranks the rows, 8-byte keys in 64 KB of LDS; a larger A is an error and launches nothing); budget >= 1,
 *     cooldown >= 0, threshold not NaN.  sel, int32 (1 + budget): sel[0] = n = min(candidates, budget), sel[1..n] = the
 *     chosen ROW POSITIONS i in ascending rank; entries after n are not written.  wait is advanced as above.  counts, (S x 2) int32 or
 *     NULL: counts[b_i][0] += cand_i, counts[b_i][1] += cand_i && !chosen_i (the candidates the budget passed over).  A row
 *     with its slot outside [0, S) is skipped whole (no candidate, no wait or counts written).
 * afx_k_cascade_windows: hdr (A x 3 int32) = slot, n, start, with n = min(samples the session has seen, window) and
 *     start = seen mod window when seen >= window, else 0.  For r < min(sel[0], budget) and i = sel[1 + r]:
 *         out[r][j] = hist[slot_i][(start_i + j) mod n_i],  j < window       (out (budget, window) fp32)
 *     -- the window oldest sample first; while n < window the history tiled, afx_k_tile_crop's function with start 0.  sel
 *     is read on the device (no read-back between select and gather); the grid covers budget rows, and rows at or past
 *     sel[0] write nothing.  Steady rows (n = window) copy four samples per lane where start and window are multiples of 4
 *     and both rows 16-byte aligned.  A row whose sel entry is outside [0, A), whose slot is outside [0, S), whose n is
 *     outside [1, window] or whose start is outside [0, n) is skipped whole.
 * A NULL pointer or a size that is not positive: non-zero, afx_last_error set, nothing launched. */
int afx_k_cascade_store(const float* x, int A, int hop, const int* hdr, float* hist, int S, int window, void* stream);
int afx_k_cascade_select(const float* scores, int stride, const int* hdr, int A, int* wait, int* counts, int S,
                         float threshold, int budget, int cooldown, int* sel, void* stream);
int afx_k_cascade_windows(const float* hist, int S, int window, const int* hdr, int A, const int* sel, int budget,
                          float* out, void* stream);
/* Verdicts (afx/verdict.py): the per-stream decision over the scores of the streaming scorers -- exponential smoothing, a
 * two-threshold hysteresis with confirm / release run lengths, and a device log of the raise / clear events.
 * Policy, all fp32 / int32: alpha in (0, 1]; enter <= exit_ and verifier_enter, none NaN; confirm, release, min_scores >= 1;
 * latch 0 / 1.  State per slot: m (S,) fp32, the smoothed score, NaN for a new stream; st (S, 4) int32 = (n, run, on, since),
 * (0, 0, 0, -1) for a new stream: n the scores taken (saturating at 2^31 - 1), run the current run length, on 0 clear / 1
 * alarm, since the hop index at which the current alarm was raised, -1 while clear.
 * An update names rows i = 0..A-1: slot b_i = hdr[i][0] (distinct), hop index k_i = hdr[i][1] (hdr: device, A x 2 int32),
 * score s_i = scores[i * stride] (fp32 bonafide score, low = spoof; stride >= 1: a column of a logits matrix is read in
 * place) and v_i = vscores[i] (the verifier's score of the slot in this push, NaN if none; vscores NULL: every v_i is NaN).
 * All compares are fp32, every arithmetic operation is a single correctly rounded fp32 operation (no fma):
 *     if (isnan(s_i)) the row changes nothing and logs nothing           (a gate's "no hop completed")
 *     n1 = n == 2^31-1 ? n : n + 1
 *     m1 = n == 0 ? s_i : m + alpha * (s_i - m)                          (sub, mul, add: three roundings)
 *     kind = 0
 *     if (on == 0) {
 *         if (!isnan(v_i) && v_i < verifier_enter) on, run, since, kind = 1, 0, k_i, 2    (raised by the verifier)
 *         else if (!isnan(v_i))                    run = 0       (the verifier cleared this window: the run starts over)
 *         else if (n1 >= min_scores && m1 < enter) { run += 1; if (run >= confirm) on, run, since, kind = 1, 0, k_i, 1 }
 *         else                                     run = 0
 *     } else if (!latch) {
 *         if (m1 >= exit_) { run += 1; if (run >= release) on, run, since, kind = 0, 0, -1, 3 }
 *         else             run = 0
 *     }
 *     m = m1; n = n1
 * Infinite scores follow IEEE; a NaN m1 is neither < enter nor >= exit_.  While an alarm is on the verifier plays no part:
 * its veto acts before the alarm, by restarting the confirm run.
 * The log, int32 (1 + 4 cap): a row with kind != 0 appends the event (b_i, kind, k_i, bits of m1); the events of one launch
 * in ascending row position, launches in stream order.  log[0] is the number of events since the log was last cleared
 * (the caller zeroes it), event e sits at log[1 + 4e ..]; events at or past cap are not stored but still counted in log[0],
 * and the state always advances.
 * afx_k_verdict: 1 <= A <= 8192, ONE workgroup of 1024 threads takes the rows in chunks of 1024 in row order (event slots
 * from a wave ballot + popcount prefix, wave totals prefixed through LDS onto a running base that starts at log[0]: no
 * atomics, no second launch).  A row whose slot is outside [0, S) is skipped whole (no state change, no event); the state
 * rows of slots not named are untouched.  A NULL scores / hdr / m / st / log, stride < 1, A outside 1..8192, S < 1, alpha
 * outside (0, 1], a NaN threshold, exit_ < enter, confirm / release / min_scores < 1, latch outside {0, 1} or cap < 0:
 * non-zero, afx_last_error names `verdict`, nothing launched. */
int afx_k_verdict(const float* scores, int stride, const float* vscores, const int* hdr, int A, float* m, int* st, int S,
                  float alpha, float enter, float exit_, float verifier_enter, int confirm, int release, int min_scores,
                  int latch, int* log, int cap, void* stream);
/* Evidence clips (afx/evidence.py): the audio and the scores around each alarm, kept on the device.  Policy: pre >= 0 hops
 * kept before the raising hop, post >= 0 hops after it, `clips` pool entries, encoding 0 = fp32 (bit for bit) / 1 = pcm16.
 * P = pre + 1, a clip holds L = P + post hops.
 * State per slot: hist (S, P hop) fp32, the audio ring; sring (S, P) fp32, the score ring; rec (S,) int32, the pool entry
 * being recorded or -1; left (S,) int32, post-roll hops still to append.  Pool: pool (clips, 6) int32 headers = (status,
 * slot, raised_at, first_hop, hops, seq), status 0 FREE / 1 RECORDING / 2 COMPLETE / 3 TRUNCATED (3 is set by the host's
 * reset alone); audio (clips, L hop) fp32 or int16; cscores (clips, L) fp32; counters (4,) int32 = raised, recorded,
 * dropped, merged.  Entries become FREE only between updates (the host's take_clips).
 * An update names rows i = 0..A-1: slot b_i = hdr[i][0] (distinct), the 1-based hop number k_i = hdr[i][1] (the host's
 * samples_seen / hop after this hop), the hop x[i][0..hop), the score s_i = scores[i * stride] (NaN if this push produced
 * none; scores NULL: every s_i is NaN) and the verdict state row vst[b_i] = (n, run, on, since), read after this push's
 * verdict update.  The update behaves as if the rows were processed in ascending row position:
 *     store:  hist[b][((k-1) mod P) hop + j] = x[i][j], j < hop;  sring[b][(k-1) mod P] = s_i
 *     raise = on == 1 && since == k                                       (raised by this very push)
 *     if (rec[b] >= 0) {                                                  (recording)
 *         merged += raise
 *         e = rec[b]; the hop, encoded, and s_i go to position hops_e of clip e; hops_e += 1; left[b] -= 1
 *         if (left[b] == 0) status_e = COMPLETE, rec[b] = -1
 *     } else if (raise) {
 *         raised += 1
 *         e = the FREE entry of lowest index not yet taken by an earlier row of this update; none: dropped += 1, and that is all
 *         f = max(1, k - pre); header_e = (post == 0 ? COMPLETE : RECORDING, b, k, f, k - f + 1, recorded); recorded += 1
 *         hops f..k (hop h from ring position (h-1) mod P, which already holds hop k), encoded, and their scores go to
 *         positions 0..k-f of clip e;  if (post > 0) rec[b] = e, left[b] = post
 *     }
 * The free set is fixed during an update, so the entry of a raising row is the (number of raising, not recording rows before
 * it)-th FREE entry in ascending index, whatever the launch geometry.  f >= 1: a ring is never read further back than the
 * session's first hop.  pcm16 of a sample x: q = x * 32768 (one fp32 multiply), NaN -> 0, q clamped to [-32768, 32767] and
 * rounded half to even, stored as int16.
 * A row with a slot outside [0, S) or k < 1 is skipped whole (nothing stored, no state change); of the rows naming one slot
 * the one at the lowest row position is taken and the others are skipped whole.
 * afx_k_evidence_mark: 1 <= A <= 8192, 1 <= clips <= 8192, ONE workgroup of 1024 threads: the FREE entries are listed in
 * LDS (ballot + popcount prefix), the rows are taken in chunks of 1024 in row order (rank of a raising row from a wave ballot
 * + popcount prefix, wave totals through LDS onto a running base).  Updates rec, left, the headers and the counters, and
 * writes work (A, 4) int32 = (op, entry, a, b): op -1 the row is skipped, 0 store only, 1 append at position a of `entry`,
 * 2 open `entry` with first hop a and b hops.  claim: (S,) int32 scratch, every word 2^31 - 1 before the first launch (the
 * kernel leaves it so): rows naming one slot settle their owner through an atomic min.
 * afx_k_evidence_copy: a grid over rows x hop tiles carries the work items out on the rings, the clips' audio and scores;
 * 128-bit accesses where hop % 4 == 0 and the rows are 16-byte aligned, one sample per lane otherwise.  A work item whose
 * entry, position or hops leave the pool (or do not end at k) is skipped whole.
 * A NULL pointer (scores excepted), A outside 1..8192, S < 1, hop < 1, pre < 0, post < 0, a ring or a clip of 2^31 samples
 * or more, clips outside 1..8192, stride < 1 with scores, encoding outside {0, 1}: non-zero, afx_last_error names
 * `evidence_mark` / `evidence_copy`, nothing launched. */
int afx_k_evidence_mark(const int* hdr, int A, const int* vst, int S, int pre, int post, int* rec, int* left, int* claim,
                        int* pool, int clips, int* counters, int* work, void* stream);
int afx_k_evidence_copy(const float* x, const float* scores, int stride, const int* hdr, const int* work, int A, int hop,
                        int pre, int post, float* hist, float* sring, int S, void* audio, float* cscores, int clips,
                        int encoding, void* stream);
/* Input quality (afx/quality.py): what the hop behind each score looked like, measured on the device, and a score that is
 * passed on or replaced by NaN ("cannot judge").  Policy, fp32 / int32: clip > 0, clip_count >= 1, flat_run >= 2, e_quiet >= 0
 * (the host's fp32(quiet * hop), product in double, rounded once), dc >= 0 (fp32(dc * hop) likewise), mask in 0..31,
 * max_bad >= 0, abstain 0 / 1; 1 <= W <= 1024 hops of window.
 * State per slot: ring (S, W) uint8, the flags of hop j at (j - 1) mod W; state (S, 3) int32 = (last, run, bad): the bits of
 * the newest sample, the length of the run of identical samples it ends, the flagged hops of the window -- (0, 0, 0) for a
 * new stream; totals (S, 6) int32, saturating at 2^31 - 1: hops seen, hops with flag 1, 2, 4, 8, 16.
 * An update names rows i = 0..A-1: slot b_i = hdr[i][0] (distinct), hop index k_i = hdr[i][1] >= 1 (the host's samples_seen /
 * hop after this hop; hdr: device, A x 2 int32), the hop x[i * stride + 0 .. hop) (fp32, stride >= hop in floats: a chunk may
 * be a view) and s_i = scores[i * sstride] (scores NULL: no scores, no out).  Every arithmetic operation is one correctly
 * rounded fp32 operation (no fma):
 *     nonfinite = #{ j : (bits(x_j) & 0x7f800000) == 0x7f800000 }
 *     clipped   = #{ j : |x_j| >= clip }                                   (fp32 compare: a NaN is not counted)
 *     peak      = max |x_j| over the x_j that are not NaN, +0.0 if none
 *     e, s      = the sum of x_j * x_j and the sum of x_j, both in this order: the hop padded with +0.0 to a multiple of 1024
 *                 and viewed as y[tile][t][c], t < 256, c < 4 (element 1024 tile + 4 t + c);
 *                 q[t][c] = y[0][t][c], then + y[1][t][c], ... in ascending tile order;
 *                 r[t] = (q[t][0] + q[t][1]) + (q[t][2] + q[t][3]);
 *                 for w = 128, 64, .., 1: r[t] = r[t] + r[t + w], t < w;  the result is r[0].
 *                 Non-finite values follow IEEE; a NaN result is recorded as 0x7fc00000 (IEEE fixes no payload)
 *     longest   = max of r_j over the hop, r_j = 1 if bits(x_j) != bits of the sample before it in the STREAM, else that
 *                 sample's r + 1 (saturating at 2^31 - 1); (last, run) carry across hops and run = 0 before a session's first
 *                 sample, so its r is 1.  The compare is bitwise: +0 and -0 differ, two NaNs of equal bits are equal
 *     flags     = 1 NONFINITE (nonfinite > 0) | 2 CLIPPED (clipped >= clip_count) | 4 FLAT (longest >= flat_run)
 *               | 8 QUIET (e < e_quiet) | 16 DC (|s| > dc);   a NaN e or s sets neither 8 nor 16
 *     ring[b][(k - 1) mod W] = flags
 *     bad       = #{ j in [max(1, k - W + 1), k] : ring[b][(j - 1) mod W] & mask }   (never before the session's first hop)
 *     state[b]  = (bits of the hop's last sample, r of it, bad);  totals[b][0] += 1, totals[b][1 + n] += (flags >> n) & 1
 *     meas[i]   = (flags, nonfinite, clipped, longest, bits(e), bits(s), bits(peak), bad)          8 int32
 *     out[i]    = s_i, bit for bit, if bad <= max_bad or abstain == 0, else the quiet NaN 0x7fc00000
 * A row with a slot outside [0, S) or k < 1 is skipped whole: no state change, meas[i] all -1, out[i] = s_i.
 * afx_k_quality: one workgroup of 256 threads per row, thread t owns y[.][t][0..3] (dwordx4 loads where x and stride are
 * 16-byte aligned and the four elements are inside the hop, element loads otherwise, the same order); the tree's w = 128 and
 * 64 steps go through LDS, w <= 32 through the wave; counts and peak are integer reductions; the run is a reduction, in stream
 * order, over an associative summary (length, first and last bits, leading run, trailing run, longest run).  No atomics.
 * A NULL x / hdr / ring / state / totals / meas, scores without out or with sstride < 1, A outside 1..8192, hop outside
 * 1..2^24, stride < hop, S < 1, W outside 1..1024 or a policy value outside the ranges above (NaN included): non-zero,
 * afx_last_error names `quality`, nothing launched. */
int afx_k_quality(const float* x, long long stride, int A, int hop, const int* hdr, const float* scores, int sstride,
                  float clip, int clip_count, int flat_run, float e_quiet, float dc, int mask, int max_bad, int abstain,
                  unsigned char* ring, int W, int* state, int* totals, int S, int* meas, float* out, void* stream);
/* Provenance (afx/provenance.py): which 16 kHz samples the jitter buffer made up, counted per frame and per hop on the
 * device, and a score that is passed on or replaced by NaN while too much of the model's window is synthetic.
 * Marks.  E is a slot's played-out stream (afx/jitter.py); C[i] = 1 where released index i was not received (loss-concealed
 * in any mode, "zero" included, or comfort noise), else 0.  Output sample K of the slot's resampled stream, counted from the
 * session's origin, has the mark c16[K] = C[floor(K * M / L)] (L / M the slot's up / down ratio; the identity: c16 = C): the
 * newest input sample of K's filter support, so a release that moves the playout counter from N to N + n_in makes exactly
 * the outputs whose source lies in [N, N + n_in), and a synthetic run [u, v) of it is the outputs [ceil(u L / M),
 * ceil(v L / M)).  The mark leads the filter's centre by the resampler's delay (0.6 to 1.25 ms); a count does not care.
 * Counts.  n[f] = the sum of c16 over the 16 kHz frame f (`frame` samples where a gate stands in the chain, else the whole
 * hop); a hop's count c = the sum of n over its frames; behind a gate the gated stream's frame counts are the kept frames'
 * counts, in order, exactly as the samples are compacted.
 * afx_k_prov_spans: psyn (device, S x ring_len bytes, parallel to a front's pending ring).  rows (device, R x 4 int32) =
 * slot, wpos, n, value: psyn[slot][(wpos + k) mod ring_len] = value for k < n.  The rows of a launch write disjoint
 * ranges; max_n >= every n sizes the grid.  A row with a slot outside [0, S), wpos outside [0, ring_len), n outside
 * [0, ring_len] or a value other than 0 / 1 is skipped whole.  Dword stores between a range's unaligned ends.
 * afx_k_prov_frames: table (device, R x 2 int32) = slot, head: out[i][f] (device, R x hop / frame int32) = the number of
 * non-zero bytes among psyn[slot][(head + f frame + k) mod ring_len], k < frame.  One wave per (row, frame), byte loads, a
 * wave-64 shuffle reduction.  A row with a bad slot or head: its out row is all -1.
 * afx_k_prov_compact: after a gate launch over A rows of F = n / frame frames (F <= 512).  counts (device, A x F int32, the
 * frame counts of the rows' hops), mask (device, A x F bytes, the gate launch's mask: bit 0 = kept), hdr (device, A x 2
 * int32) = slot, wpos (the gate launch's own header: the slot's write position in samples, a multiple of frame).  gsyn
 * (device, S x ring_frames int32, parallel to the gate's pending ring): the counts of the kept frames, in order, to
 * gsyn[slot][(wpos / frame + r) mod ring_frames], r = 0, 1, ...  One workgroup per row: an exclusive scan of bit 0, then a
 * scatter.  A row with a bad slot or wpos, or with a count outside [0, frame], is skipped whole.
 * afx_k_prov_take: table (device, R x 2 int32) = slot, head (the pop's own table: the ring head in samples, a multiple of
 * frame): out[i] = the sum of gsyn[slot][(head / frame + k) mod ring_frames], k < per (saturating at 2^31 - 1); -1 for a row
 * with a bad slot or head, or with a negative entry.  One wave per row.
 * afx_k_provenance, the layer update.  1 <= W <= 1024 hops of window, 1 <= hop <= 2^24, 0 <= limit <= W * hop (the host's
 * floor(float64(fp32(max_share)) * W * hop)), abstain 0 / 1.  State per slot: ring (S, W) int32, the count of hop j at
 * (j - 1) mod W; state (S, 2) int32 = (total, valid), (0, 1) for a new stream; totals (S, 3) int32 saturating at 2^31 - 1 =
 * hops, synthetic samples, hops that were not valid.  Rows i = 0..A-1, A <= 8192: slot b_i = hdr[i][0] (distinct), hop index
 * k_i = hdr[i][1] >= 1 (hdr: device, A x 2 int32), c_i = counts[i] in [0, hop] (device, A int32), s_i = scores[i * sstride]
 * (scores NULL: no scores, no out):
 *     ring[b][(k - 1) mod W] = c
 *     total    = the sum of ring[b][(j - 1) mod W] over j in [max(1, k - W + 1), k]   (never before the session's first hop)
 *     valid    = total <= limit;   state[b] = (min(total, 2^31 - 1), valid)
 *     totals[b] += (1, c, 1 - valid)
 *     meas[i]  = (c, min(total, 2^31 - 1), valid)                                      3 int32
 *     out[i]   = s_i, bit for bit, if valid or abstain == 0, else the quiet NaN 0x7fc00000
 * A row with a slot outside [0, S), k < 1 or c outside [0, hop] is skipped whole: no state change, meas[i] all -1, out[i] =
 * s_i.  One thread per row, the recount a loop over at most W entries.
 * Every entry point: a NULL pointer (scores and its out excepted) or a scalar outside the ranges above (S < 1, rows outside
 * 1..65535 -- take: 1..262140, provenance: 1..8192 --, a ring longer than 2^30, hop > ring_len, hop % frame != 0, per >
 * ring_frames, F > ring_frames): non-zero, afx_last_error names `prov_spans` / `prov_frames` / `prov_compact` / `prov_take` /
 * `provenance`, nothing launched. */
int afx_k_prov_spans(unsigned char* psyn, int S, int ring_len, const int* rows, int R, int max_n, void* stream);
int afx_k_prov_frames(const unsigned char* psyn, int S, int ring_len, const int* table, int R, int hop, int frame, int* out,
                      void* stream);
int afx_k_prov_compact(const int* counts, const unsigned char* mask, const int* hdr, int A, int F, int frame, int* gsyn, int S,
                       int ring_frames, void* stream);
int afx_k_prov_take(const int* gsyn, int S, int ring_frames, const int* table, int R, int per, int frame, int* out,
                    void* stream);
int afx_k_provenance(const int* hdr, const int* counts, const float* scores, int sstride, int A, int hop, long long limit,
                     int abstain, int* ring, int W, int* state, int* totals, int S, int* meas, float* out, void* stream);
/* Provenance behind a look-ahead gate and through turns (afx/provenance.py, ProvenancePolicy(through="all")).  n[f] is the
 * count of gate frame f of the stream the gate was pushed, 0 <= n[f] <= frame.  All integer arithmetic, exact.
 * Behind afx_k_gate_la the gated stream is the emitted frames in order (keep'), so its frame counts are n[g] over the emitted
 * g, in order.  State per slot: gline (device, S x pre int32), the count of delayed frame g at block g mod pre, parallel to
 * `line`; a reset leaves it alone (nothing before the session's first frame is ever read).
 * afx_k_prov_compact_la: directly after an afx_k_gate_la launch over A rows of n_frames frames, with that launch's own header
 * and mask.  hdr (device, A x 4 int32) = slot, wpos (samples, on the frame grid), F (frames pushed before this row), 0;
 * counts (device, A x n_frames int32): the counts of frames F .. F + n_frames - 1; mask (device, A x n_frames bytes): entry j =
 * keep' of frame F - pre + j.  Per row, r = 0; for j = 0 .. n_frames - 1 with g = F - pre + j:
 *     if g >= 0 and mask[j] & 1:
 *         c = j < pre ? gline[slot][g mod pre] : counts[j - pre]
 *         gsyn[slot][(wpos / frame + r) mod ring_frames] = c;   r += 1
 * then for i = max(0, n_frames - pre) .. n_frames - 1:   gline[slot][(F + i) mod pre] = counts[i]
 * (every read of gline precedes every write of the row: frame G enters the block frame G - pre leaves).  A row with a slot
 * outside [0, S), wpos outside the ring or off the frame grid, F < 0, F + n_frames >= 2^31 or a count outside [0, frame] is
 * skipped whole, nothing written.  One workgroup per row: an exclusive scan of mask bit 0 (the device function
 * afx_k_prov_compact scans with), then a scatter.  afx_k_prov_take serves the pop unchanged.  A NULL pointer, A outside
 * 1..65535, n_frames outside 1..512 or above ring_frames, pre outside 1..31, frame <= 0, S < 1 or a ring above 2^30:
 * non-zero, afx_last_error names `prov_compact_la`, nothing launched.
 * Through turns: afx_k_turn copies kept frame j of a row to bufs[slot][open][n]; bsyn (device, S x 2 x max_frames int32,
 * parallel to bufs in frames) takes counts[j] at the same place (the turn mask is not delayed).  Entries beyond an open or
 * completed turn's frames are undefined, as in bufs.
 * afx_k_prov_turn: directly BEFORE afx_k_turn on the same stream, with the same mask (A x F) and header (A x 3 = slot, wpos,
 * g0) and counts (device, A x F int32).  It reads state (open, n) and never writes it, replays afx_k_turn's recurrence for
 * open and n only and stores the kept frames' counts where that recurrence stores the frames (those of a turn the row drops
 * as short are not stored).  It skips the rows afx_k_turn skips (slot, g0, a state that is no turn state) plus any row with
 * a count outside [0, frame]; it is not told the staging ring's length, so of wpos it checks wpos >= 0 only.  It refuses
 * the scalars afx_k_turn refuses (the ring length excepted), by name (`prov_turn`).  One wave per row.
 * afx_k_prov_turn_sum: beside afx_k_turn_collect, over the same table rows (device, R x 3 int32) = slot, buffer, frames m:
 *     q = max_frames / m, rem = max_frames % m;   out[i] = q * sum(bsyn[slot][buffer][0..m)) + sum(bsyn[slot][buffer][0..rem))
 * the count of the turn tiled to max_frames frames (saturating at 2^31 - 1; with entries <= frame it is at most the window).
 * out[i] = -1 for a row afx_k_turn_collect would skip (slot outside [0, S), buffer not 0 / 1, m outside 1..max_frames) or with
 * a negative entry among those it reads.  One wave per row, a wave-64 shuffle reduction of the two partial sums, no
 * atomics.  A NULL pointer, S < 1, max_frames < 1 or R outside 1..262140: non-zero, `prov_turn_sum`, nothing launched. */
int afx_k_prov_compact_la(const int* counts, const unsigned char* mask, const int* hdr, int A, int n_frames, int frame, int pre,
                          int* gline, int* gsyn, int S, int ring_frames, void* stream);
int afx_k_prov_turn(const int* counts, const unsigned char* mask, const int* hdr, int A, int F, int frame, int min_frames,
                    int max_frames, const int* state, int* bsyn, int S, void* stream);
int afx_k_prov_turn_sum(const int* bsyn, int S, int max_frames, const int* rows, int R, int* out, void* stream);
/* Row LayerNorm (+ activation) of fp32 rows: 0 < C <= 1024, C % 4 == 0, any rows >= 1; out_f and / or out_h.  ldx, ldo_f,
 * ldo_h count elements (>= C).  A lane reads and writes 4 columns at a time, so rows must be aligned to that access: x,
 * gamma, beta, out_f 16-byte aligned with ldx % 4 == 0 and ldo_f % 4 == 0; out_h 8-byte aligned (16 for the fp32 operand
 * types) with ldo_h % 4 == 0.  A violation: non-zero, afx_last_error names `rownorm`, nothing launched. */
int afx_k_rownorm(int dtype, const float* x, long ldx, int rows, int C, const float* gamma, const float* beta,
                  float eps, int act, float* out_f, long ldo_f, void* out_h, long ldo_h, void* stream);
int afx_k_mhsa(int dtype, const void* qkv, void* out, int B, int T, int H, void* stream);
int afx_k_conf_attn(int dtype, const float* q, long ldq, const float* kv, long ldkv, const float* rel, int max_pos,
                    int B, int N, int H, int dh, void* out_h, long ldo, void* stream);
/* the same on the matrix cores (operand-type q/k/E/P, fp32 accumulation): rel_h is the embedding table
 * packed by afx_k_pack_linear with Kpad = 64; head dim 36, at most 209 tokens */
int afx_k_conf_attn_mfma(int dtype, const float* q, long ldq, const float* kv, long ldkv, const void* rel_h, int max_pos,
                         int B, int N, int H, int dh, void* out_h, long ldo, void* stream);
int afx_k_conf_dwconv(int dtype, const float* x, long ldx, const float* w, const float* bias, const float* bn_scale,
                      const float* bn_shift, int B, int N, int C, int k, void* out_h, long ldo, void* stream);

/* ---- AASIST graph modules alone (models/aasist_modules.py:17-110, 112-294, 296-338);
 * all fp32, BatchNorm passed folded (scale = w/sqrt(var+eps), shift = b - mean*scale).
 * Supported (in,out) dims: (64,64), (64,32), (32,32); N <= 80 nodes. ------------------ */
const char* afx_aasist_error(void);
int afx_k_gat(const float* x, int B, int N, int din, int dout, const float* att_w, const float* att_b,
              const float* att_vec, const float* w1, const float* b1, const float* w2, const float* b2,
              const float* bn_scale, const float* bn_shift, float temp, float* y, void* stream);
/* wts: t1w t1b t2w t2b att_w att_b attM_w attM_b v11 v22 v12 vM w1 b1 w2 b2 w1M b1M w2M b2M bn_scale bn_shift
 * master == NULL -> mean of the projected nodes; xp_scratch: B*(n1+n2)*din + B*din floats */
int afx_k_hgat(const float* x1, int n1, const float* x2, int n2, int B, int din, int dout, const float* const* wts,
               float temp, const float* master, long master_bstride, float* xp_scratch, float* y1, float* y2,
               float* mout, void* stream);
int afx_k_graph_pool(const float* h, int B, int N, int D, int keep, const float* w, const float* b, float* out,
                     void* stream);

/* Residual_block alone (models/aasist_modules.py:340-397: conv1 (2,3) pad (1,1) ON x (Q2) -> bn2 -> SELU -> conv2 (2,3)
 * pad (0,1), + conv_downsample (1,3) of x when the channel count changes).  x, y: device NCHW fp32 (B,cin,H,W) /
 * (B,cout,H,W); conv weights in their checkpoint layout [cout][cin][kh][kw]; bn2 folded; down_w/down_b NULL exactly when
 * cin == cout.  cin 1 or a multiple of 16, cout 32 / 64 / 128.  scratch: afx_k_resblock_scratch_floats() floats. */
size_t afx_k_resblock_scratch_floats(int B, int cin, int cout, int H, int W);
int afx_k_resblock(const float* x, int B, int cin, int cout, int H, int W, const float* conv1_w, const float* conv1_b,
                   const float* bn2_scale, const float* bn2_shift, const float* conv2_w, const float* conv2_b,
                   const float* down_w, const float* down_b, float* scratch, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AFX_H_ */
