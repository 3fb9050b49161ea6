/*
 * casapose_hip.h -- C ABI of libcasapose_hip.so (gfx950 / MI355X).
 *
 * The reference (fraunhoferhhi/casapose) has no FFI: its hot path bottoms out in
 * TensorFlow / tensorflow-addons ops.  Each entry point below replaces the native
 * work behind one group of reference call sites (cited as file:line relative to the
 * reference tree).  The Python host (casapose_amd/) binds these with ctypes; a
 * maintainer of the reference would bind them the same way.
 *
 * Conventions
 *   - every function returns 0 on success, a negative cp_status otherwise; nothing
 *     throws across the boundary; cp_last_error() returns a thread-local message.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns
 *     every buffer (inputs, outputs, workspaces); no hidden allocation.
 *   - `stream` is a hipStream_t passed as void* (0 = null stream); calls are
 *     asynchronous with respect to the host and re-entrant across streams.
 *   - tensors are NHWC, fp32 unless stated; label maps are uint8 (0 = background).
 */
#ifndef CASAPOSE_HIP_H
#define CASAPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cp_status {
    CP_OK = 0,
    CP_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    CP_ERR_LAUNCH = -2,    /* hipLaunch / runtime failure */
    CP_ERR_NO_DEVICE = -3
} cp_status;

const char* cp_last_error(void);
/* ABI version of the library: CP_ABI_VERSION of the header it was built from.  300 (round 3): cp_conv_desc starts with `struct_size`
 * and every entry point that takes a descriptor refuses one whose struct_size differs from the library's sizeof(cp_conv_desc)
 * (CP_ERR_INVALID, message in cp_last_error()) instead of reading fields a shorter or longer caller-side struct does not have.
 * 301 (round 6): + the f16x2 range-guard entry points (cp_f16x2_monitor_set / _get, cp_f16x2_range_check, cp_amax_f32); no struct changed.
 * 302 (round 6): cp_conv_desc ends with head_prefix / head_prefix_n / head_prefix_ld (whole output records from the last fused head). */
#define CP_ABI_VERSION 302
int cp_version(void);
/* sizeof(cp_conv_desc) / sizeof(cp_conv_source) as this library was compiled: a binder checks them against its own declaration at load time */
size_t cp_conv_desc_size(void);
size_t cp_conv_source_size(void);
/* Blocks of the PERSISTENT convolution / GEMM launches (csrc/conv_hsplit.hip, csrc/wino_gemm_split.hip): 256 = one per CU (default; the
 * environment variable CASAPOSE_PERSIST_BLOCKS sets the initial value).  A smaller multiple of 8 leaves whole CUs free, so that an HBM-bound
 * kernel launched on ANOTHER stream runs beside the matrix-pipe kernel instead of behind it -- the two-stream forward of the host layer sets 224
 * around its launches.  Process-wide, read at launch time on the calling thread. */
int cp_set_persistent_blocks(int blocks);
int cp_get_persistent_blocks(void);
/* number of visible gfx950 devices (0 on a CPU-only host); never initialises a context */
int cp_device_count(void);
/* Matrix-pipe probe (measurement aid, bench.py): one launch of a bare MFMA stream on every SIMD -- which = 0: v_mfma_f32_32x32x2_f32,
 * 1: v_mfma_f32_32x32x16_bf16 -- so that the rate the part SUSTAINS under its power limit can be printed beside the datasheet peak the
 * roofline entries use.  ws: cp_mfma_probe_workspace_bytes() of device memory; *flops receives the FLOPs of the launch (host memory). */
size_t cp_mfma_probe_workspace_bytes(void);
int cp_mfma_probe(int which, int iters, void* ws, double* flops, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused implicit-GEMM convolution, forward, fp32 on v_mfma_f32_32x32x2_f32.
 *
 * Replaces: layers.Conv2D in the encoder (casapose/pose_models/models/resnet.py:85-87,
 * 97-99,103,249) and decoder 1 (models/casapose.py:71-74, pose_models.py:546,616);
 * PartialConvolution.calc (models/_normalization_layers.py:325-373);
 * inference-mode SyncBatchNormalization + ReLU / leaky pair (resnet.py:78-79,100-101,
 * 250-251,303-304; casapose.py:77,98-107); ClassAdaptiveWeightedNormalization.calc
 * (_normalization_layers.py:119-139); layers.Add (resnet.py:110); layers.concatenate
 * (pose_models.py:542-545,571,583,595,607); GuidedUpsampling gather
 * (_normalization_layers.py:554-558) and UpSampling2D(bilinear) (casapose.py:135-140)
 * when fused into the consumer's operand load.
 *
 *  out[n,oy,ox,co] = EPI( sum_{s in sources} sum_{ky,kx} sum_c
 *                         A_s(n, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad, c) * Wp[co, k(s,ky,kx,c)] )
 *
 *  A_s(n,y,x,c) is 0 outside [0,in_h)x[0,in_w), else the source value fetched through
 *  the source's spatial mode, optionally (source 0/1 individually) passed through a
 *  per-channel affine `v*pre_scale[c]+pre_shift[c]`, and, when `tap_label` is set,
 *  multiplied by [tap_label[n,y,x] == tap_label[n,oy,ox]] (partial convolution; needs
 *  stride 1 so both live on the same grid).
 *
 *  EPI(v): v *= row_scale[n,oy,ox] (partial-conv 9/count)      if row_scale
 *          v += residual[n,oy,ox,co]                           if residual
 *          out_raw = v                                         if out_raw
 *          t = v*sc + sh ; (sc,sh) = (scale[co],shift[co]) or, if epi_label,
 *                          (scale[epi_label[n,oy,ox]*cout+co], shift[...])   (CLADE table)
 *          t = act(t): 0 none, 1 relu, 2 leaky 0.1 (relu(t)-relu(-0.1t))
 *          out_act = t                                         if out_act
 *
 *  Packed weights Wp: row-major [cout][ktot] fp32, produced by cp_conv_pack_weights
 *  (K order: source 0 chunks, then source 1 chunks; see cp_conv_ktot).
 * ---------------------------------------------------------------------------------- */

enum { CP_SRC_DIRECT = 0, CP_SRC_NEAREST_SEL = 1, CP_SRC_BILINEAR_X2 = 2,
       CP_SRC_ZERO_INSERT_X2 = 3 /* the source holds the EVEN positions of the in_h x in_w grid, the rest is zero:
                                    the data-gradient of a stride-2 convolution (transposed convolution) */ };
enum { CP_ACT_NONE = 0, CP_ACT_RELU = 1, CP_ACT_LEAKY01 = 2 };

typedef struct cp_conv_source {
    const float* data;      /* NHWC, pixel stride `ld` floats                                 */
    int channels;           /* multiple of 32, or exactly 4 ("C4" mode: 8 taps per K chunk)  */
    int ld;                 /* floats between consecutive pixels (>= channels)               */
    int mode;               /* CP_SRC_*: DIRECT reads an in_h x in_w grid; the X2 modes read  */
                            /* an (in_h/2) x (in_w/2) grid                                   */
    const uint8_t* sel;     /* CP_SRC_NEAREST_SEL: [n,in_h,in_w] neighbour index 0..3         */
    const float* pre_scale; /* optional per-channel affine applied to in-bounds values       */
    const float* pre_shift;
} cp_conv_source;

typedef struct cp_conv_desc {
    uint32_t struct_size;       /* = sizeof(cp_conv_desc) of the header the CALLER was built against; checked by every entry point */
    int batch, in_h, in_w;      /* conv-input grid (after any fused x2 upsampling)           */
    int out_h, out_w, cout;
    int kh, kw, stride, dilation, pad;
    int num_sources;            /* 1 or 2 (channel concatenation, source 0 first)            */
    cp_conv_source src[2];
    const float* weights;       /* packed [cout][ktot]                                        */
    const float* weights_halo;  /* optional second packing (cp_conv_pack_weights_halo_host): lets 3x3/s1/p1   */
                                /* layers with cout <= 64 (a multiple of 4; outputs / residual 16-byte aligned  */
                                /* with ld % 4 == 0) run on the LDS-resident halo-tile kernel                 */
    const uint8_t* tap_label;   /* optional [n,in_h,in_w] -> partial-conv tap mask            */
    /* epilogue */
    const float* row_scale;     /* optional [n,out_h,out_w]                                   */
    const float* residual;      /* optional NHWC, pixel stride residual_ld                    */
    int residual_ld;
    const float* scale;         /* optional [cout] or [classes][cout] with epi_label          */
    const float* shift;
    const uint8_t* epi_label;   /* optional [n,out_h,out_w]                                   */
    int act;                    /* CP_ACT_* applied to out_act only                          */
    float* out_raw;             /* optional, pixel stride out_raw_ld                          */
    int out_raw_ld;
    float* out_act;             /* optional, pixel stride out_act_ld                          */
    int out_act_ld;
    int tile_hint;              /* 0 = auto; otherwise a CP_TILE_* value (benchmark / tests) */
    /* optional fused 1x1 head (halo-tile kernel only, cout == 32): head_out[n,y,x,0..head_cout) = sum_c out_act[..,c] *
     * Wh[c][q]; replaces pv_final_conv_segmentation / pv_final_conv_vertex (pose_models.py:546,616).  head_weights from
     * cp_conv_pack_head_weights_host.  With a head, out_act/out_raw may both be NULL (the 32-channel tensor is not stored). */
    const float* head_weights;
    float* head_out;
    int head_cout, head_out_ld;
    /* optional grouped GEMM (the 36 Winograd planes in one launch): output pixels [g*group_rows, (g+1)*group_rows) use the
     * packed weights at weights + g*group_weight_stride floats.  group_rows must be a multiple of 128; 0 = ungrouped. */
    int group_rows, group_weight_stride;
    /* optional, with a fused head: head_label_out[n,y,x] = arg-max over the first head_label_classes head channels of the pixel (uint8; first
     * maximum wins, as cp_argmax_labels) -- the hard label map of pose_models.py:547-554 straight from the head's registers */
    uint8_t* head_label_out;
    int head_label_classes;
    /* optional, with a fused head (round 6, ABI 302; cp_conv2d_fwd_split* with a head-only layer): whole output RECORDS.  head_out then addresses the
     * record of a pixel (stride head_out_ld, 16-byte aligned); its floats [0, head_prefix_n) are copied from head_prefix[pixel * head_prefix_ld + j]
     * (dense rows another head wrote), the head's channel q goes to float head_prefix_n + q.  Two heads that each write a slice of the records
     * leave every 128-byte line partly written, which costs the memory system a read-modify-write; with this the last head writes whole lines.
     * 8 <= head_prefix_n <= 12.  NULL: head_out addresses the head's first column, as before. */
    const float* head_prefix;
    int head_prefix_n, head_prefix_ld;
} cp_conv_desc;

enum { CP_TILE_AUTO = 0, CP_TILE_128x128 = 1, CP_TILE_64x128 = 2, CP_TILE_128x64 = 3, CP_TILE_128x32 = 4,
       CP_TILE_64x64 = 5, CP_TILE_256x32 = 6, CP_TILE_HALO = 7 /* halo-tile kernel (needs weights_halo) */,
       CP_TILE_STEM = 8 /* 7x7/s2 4->64 stem kernel (weights_halo = cp_conv_pack_weights_stem_host packing) */ };

/* K extent (multiple of 32) of the packed weight rows for a conv with the given sources */
int cp_conv_ktot(int kh, int kw, int num_sources, const int* channels);
/* HOST helper: pack a Keras-layout kernel into Wp.  `layout` 0 = HWIO [kh][kw][cin][cout]
 * (layers.Conv2D), 1 = IHWO [cin][kh][kw][cout] (PartialConvolution.conv_w,
 * _normalization_layers.py:314-319).  cin = sum of real source channels; a source with
 * channels==4 in the descriptor may carry `real_channels[s]` < 4 real input channels.
 * dst has cout*ktot floats.  All pointers are host memory. */
int cp_conv_pack_weights_host(const float* w_host, int layout, int kh, int kw, int cout, int num_sources,
                              const int* channels, const int* real_channels, float* dst_host);
/* halo-kernel weight layout [chunk][tap][32 or 64][kc]: float count and HOST packing (3x3 kernels only) */
int cp_conv_halo_weight_floats(int cout, int num_sources, const int* channels);
int cp_conv_pack_weights_halo_host(const float* w_host, int layout, int cout, int num_sources, const int* channels,
                                   const int* real_channels, float* dst_host);
/* packing for the stem kernel (csrc/conv_stem.hip: 7x7 / stride 2 / pad 3, one 4-channel source, cout = 64), passed in
 * cp_conv_desc.weights_halo: 12800 floats [25 two-tap steps][2][64][4]; layout as for cp_conv_pack_weights_host */
int cp_conv_pack_weights_stem_host(const float* w_host, int layout, int real_channels, float* dst);
/* HOST: pack a [1][1][32][head_cout] (HWIO) 1x1 kernel for the fused head: 1024 floats */
int cp_conv_pack_head_weights_host(const float* w_host, int head_cout, float* dst_host);
int cp_conv2d_fwd_f32(const cp_conv_desc* desc, void* stream);
/* which CP_TILE_* instantiation cp_conv2d_fwd_f32 will launch for this descriptor (profiling aid) */
int cp_conv_selected_tile(const cp_conv_desc* desc);

/* ------------------------------------------------------------------------------------
 * The same convolution on the bf16 matrix pipe (csrc/conv_hsplit.hip), for the shallow high-resolution layers: 3x3 / stride 1 /
 * pad 1, cout <= 512 (a multiple of 4; channels beyond 64 in passes of 64), sources with 16-multiple channels plus an optional trailing 4-channel source (the image); source 0 may be
 * CP_SRC_BILINEAR_X2 or (with tap_label) CP_SRC_NEAREST_SEL, the fused upsamplings of the decoders; a fused 1x1 head as in cp_conv2d_fwd_f32.
 * Replaces the same reference call sites as cp_conv2d_fwd_f32 for those layers (models/casapose.py:61-82, resnet.py:97-103 stage 1).
 *   planes = 3: fp32-EQUIVALENT -- every fp32 operand is split exactly into three bf16 terms and six bf16 products are accumulated in fp32
 *               (error <= that of the fp32 MFMA); the default of the training plan, opt-in for inference
 *   planes = 1: operands rounded to bf16 (nearest even), fp32 accumulation -- "bf16 convolutions" (BASELINE.json configs[2]); 3e-2 gates
 * The descriptor is the one of cp_conv2d_fwd_f32 (tensors stay fp32 in HBM; desc->weights / weights_halo are ignored); epilogue:
 * row_scale (partial-conv 9/count, computed from tap_label), residual, out_raw, affine / CLADE table + activation -> out_act.
 * Weights: cp_conv_pack_weights_split_host lays a Keras kernel out as the fp32 image of the kernel's fragment stream
 * (cp_conv_split_weight_floats floats); cp_conv_split_weights_f32 turns that image into the bf16 planes
 * (cp_conv_split_weight_bytes bytes) on the device -- one gather + one launch re-packs after an optimizer step.
 * ---------------------------------------------------------------------------------- */
enum { CP_PLANES_F16X2 = 0x12 };   /* `planes` code of the fp16 two-way split (two planes; see cp_wino_gemm_split_scaled_f32) */
float cp_f16x2_weight_scale(float max_abs);   /* the power of two that brings max |w| into [2^11, 2^12) */
/* ---- the f16x2 RANGE GUARD behind the C ABI (round 6; the load path it protects: test_casapose.py:225-228 followed by model(img, training=False)) ----
 * The fp16 two-way split reproduces an fp32 operand to one ulp only while max |operand| of the converted tensor stays inside a band
 * ([0.5, 65504 / 4]).  WEIGHTS are brought there by cp_f16x2_weight_scale; ACTIVATIONS are measured on the device:
 *   - a MONITOR SLOT is four 32-bit words of device memory, 16-byte aligned, zeroed by the caller:
 *       [0] bits of max |x| over every fp32 value the armed launches converted to an fp16 pair (atomic max of the bit pattern), [1] number of
 *       launches that reported, [2] the same maximum for the operand of a fused 1x1 head (exists in registers only), [3] the OVERFLOW GUARD:
 *       bits 0-30 a threshold the caller writes (the bit pattern of a positive float, 0 = none), bit 31 set by the device when a report of
 *       word [0] -- by a reporting launch below or cp_amax_f32 -- exceeds it, or when cp_conv2d_wgrad_split with CP_PLANES_F16X2 converts a
 *       dY value above it (that launch reports into word [3] only).  A threshold of 65504 on the operand as converted catches every conversion
 *       that MODE.FP16_OVFL clamps in the reporting launches (inf included; NaN passes a conversion as NaN and is not flagged) -- with one
 *       exception: the OTHER operands of cp_conv2d_wgrad_split (the layer input X and the 4-channel image) are not guarded there; they are the
 *       forward's converted operands, watched by the forward's own slot.  Bit 31 stays set until the caller clears it;
 *   - cp_f16x2_monitor_set(slot) arms `slot` for the CALLING THREAD's following launches (NULL disarms).  Reporting launches:
 *       cp_conv2d_fwd_split_scaled / cp_conv2d_fwd_stem_split_scaled with CP_PLANES_F16X2 (what their loaders convert: the sources through the
 *       stem's input affine; the low-resolution source of a bilinear x2 input, which bounds its interpolation; word [2]: the fused head's operand),
 *       cp_wino_gemm_split_scaled_f32 with CP_PLANES_F16X2 (every row of V: arm it for a plain 1x1 GEMM only -- the padding rows of Winograd
 *       planes hold stale data), cp_wino_input_transform_f32 / _pre_f32 and cp_wino_output_input_transform_f32 (the planes V they WRITE: arm
 *       these, not the GEMM, for a Winograd layer).  A slot is sticky: maxima accumulate over launches and forwards until the caller zeroes it.
 *       An un-armed launch pays one uniform branch per staged slice;
 *   - cp_amax_f32 folds max |x| of a caller's own strided tensor into slot[0] (same atomic), for operands no kernel above converts;
 *   - cp_f16x2_range_check(amax, lo, hi, &rescale): 0 = inside [lo, hi] (or amax == 0), 1 = multiply the operand by the power of two *rescale
 *       (amax * rescale in [2^10, 2^11)) and the consumer's accumulator factor by its inverse -- exact; for V through
 *       cp_wino_input_transform_pre_f32's per-channel scale, for a fused head through the normalisation table feeding its (positively homogeneous)
 *       activation and head_descale --, 2 = no power of two in [2^-24, 2^24] helps or amax is not finite: run the layer with planes = 3.
 * Protocol of the host layer (casapose_amd/engine.py, ForwardPlan): a plan's first forward runs armed, reads the slots back (one synchronisation),
 * applies the remedies and repeats until every layer is in the band; afterwards every CASAPOSE_F16X2_MONITOR_EVERY-th forward runs armed, the
 * slots are copied to pinned host memory asynchronously and judged at the start of a later forward -- no synchronisation on the hot path; a slot
 * outside the band re-arms the calibration and raises one warning. */
int cp_f16x2_monitor_set(uint32_t* slot);
uint32_t* cp_f16x2_monitor_get(void);
int cp_f16x2_range_check(float amax, float lo, float hi, float* rescale);
int cp_amax_f32(const float* x, long long groups, long long group_stride, long long count, uint32_t* slot, void* stream);
int cp_conv_split_applicable(const cp_conv_desc* desc);   /* 1 if cp_conv2d_fwd_split covers this descriptor */
int cp_conv_split_weight_floats(int cout, int num_sources, const int* channels);
size_t cp_conv_split_weight_bytes(int cout, int num_sources, const int* channels, int planes);
int cp_conv_pack_weights_split_host(const float* w_host, int layout, int cout, int num_sources, const int* channels,
                                    const int* real_channels, float* dst_host);
int cp_conv_split_weights_f32(const float* packed, long long floats, int planes, void* out, void* stream);
/* HOST: a [1][1][32][head_cout] 1x1 kernel as the fp32 image (1024 floats) of the fused head's fragments; cp_conv_split_weights_f32
 * makes its planes.  head_weights_split may be NULL when desc->head_out is NULL. */
int cp_conv_pack_head_split_host(const float* w_host, int head_cout, float* dst_host);
int cp_conv2d_fwd_split(const cp_conv_desc* desc, const void* weights_split, const void* head_weights_split, int planes, void* stream);
/* planes = CP_PLANES_F16X2 (see cp_wino_gemm_split_scaled_f32 below for the arithmetic): the weight image is multiplied by `scale` (a power of two,
 * cp_f16x2_weight_scale(max |w|)) before its fp16 split, the convolution multiplies its accumulators by w_descale = 1 / scale (the fused head's by
 * head_descale, the inverse of the head image's scale).  With planes = 1 / 3 the factors must be 1 and the calls equal the two above. */
int cp_conv_split_weights_scaled_f32(const float* packed, long long floats, int planes, float scale, void* out, void* stream);
int cp_conv2d_fwd_split_scaled(const cp_conv_desc* desc, const void* weights_split, const void* head_weights_split, int planes, float w_descale,
                               float head_descale, void* stream);
/* Direct convolution with bf16 OPERANDS for the deep 3x3 layers (round 3; BASELINE.json configs[2] "bf16 convs"; csrc/conv_bf16d.hip): 3x3 / stride 1,
 * pad = dilation in {1, 2, 4}, one or two direct sources of 16-multiple channels, cout a multiple of 128 (<= 512), fp32 tensors in HBM, operands
 * rounded to bf16 (nearest even) while staged, fp32 accumulation on v_mfma_f32_32x32x16_bf16.  Epilogue: + residual, out_raw and / or
 * out_act = act(raw * scale[c] + shift[c]) with per-channel tables (no labels / tap masks / heads).  weights_bf16 = the ONE-plane
 * fragment stream of cp_conv2d_fwd_split (cp_conv_pack_weights_split_host + cp_conv_split_weights_f32(planes = 1)).  NOT fp32-equivalent:
 * gates 3e-2 of the output range against the fp32 convolution, 2e-5 against the convolution of the bf16-rounded operands. */
int cp_conv_bf16_deep_applicable(const cp_conv_desc* desc);
int cp_conv2d_fwd_bf16_deep(const cp_conv_desc* desc, const void* weights_bf16, void* stream);

/* ------------------------------------------------------------------------------------
 * Small streaming kernels around the convolutions
 * ---------------------------------------------------------------------------------- */

/* [n,h,w,3] -> [n,h,w,4] (4th channel 0): operand layout for the C4 source mode.
 * Replaces nothing arithmetic; feeds conv0 (resnet.py:247-249) and blocks 5/10
 * (pose_models.py:545,607). */
int cp_pad_channels_3to4(const float* src, float* dst, long long pixels, void* stream);

/* ZeroPadding2D(1) + MaxPooling2D(3x3, stride 2) (resnet.py:253-254) with an optional fused
 * per-channel affine + ReLU of the consumer's BatchNorm (resnet.py:78-79).  channels % 4 == 0. */
int cp_maxpool3x3s2_f32(const float* src, int batch, int h, int w, int channels, const float* scale,
                        const float* shift, int relu, float* dst, void* stream);

/* UpSampling2D(size 2, bilinear) == tf.image.resize half-pixel centres (casapose.py:135-140).
 * Stand-alone form; channels % 4 == 0. */
int cp_upsample_bilinear_x2_f32(const float* src, int batch, int h, int w, int channels, float* dst,
                                void* stream);

/* GuidedUpsampling gather (_normalization_layers.py:554-565), stand-alone form, given the
 * neighbour-selection map from cp_label_pyramid.  src [n,h,w,c] -> dst [n,2h,2w,c]. */
int cp_guided_upsample_x2_f32(const float* src, const uint8_t* sel, int batch, int h, int w, int channels,
                              float* dst, void* stream);

/* Front end of ransac_voting_layer_all_masks (ransac_voting.py:276-301): object masks [b,h,w,objects] (float, > 0.5 = inside, no background
 * channel) -> uint8 label map (highest such object index + 1; 0 = none) and counts[b][objects] = pixels inside each mask. */
int cp_mask_to_labels_f32(const float* mask, int batch, int h, int w, int objects, uint8_t* labels, int32_t* counts, void* stream);

/* arg-max over `classes` contiguous values per pixel (pixel stride ld) -> uint8 label.
 * Replaces softmax(1e6*x) as a hard one-hot (pose_models.py:547-554; voting_layers_2d.py:38-41).
 * First maximum wins (ties are undefined behaviour in the reference).
 * Two routes, one result: 16-byte loads when ld % 4 == 0, `logits` is 16-byte aligned, classes <= 12 and 4 * ceil(classes / 4) <= ld
 * (the values of the record past `classes` are loaded and ignored); a scalar loop otherwise.  1 <= classes <= 255, ld >= classes. */
int cp_argmax_labels(const float* logits, int ld, int classes, long long pixels, uint8_t* labels,
                     void* stream);

/* Everything decoder 2 derives from the label map (pose_models.py:556-559;
 * _normalization_layers.py:294-299,333-352,512-551):
 *   levels 0..3 = full, 1/2, 1/4, 1/8 resolution (HalfSize == [::2,::2]);
 *   labels[l]    uint8 [n,h_l,w_l]                 (labels[0] is the INPUT)
 *   pnorm[l]     float [n,h_l,w_l]  9 / #{3x3 taps in bounds with the centre's label}
 *   sel[l]       uint8 [n,h_l,w_l]  for l = 0..2: which neighbour of level l+1 the guided
 *                                   upsampling picks for each pixel of level l (0..3)
 * Any output pointer may be NULL.  h, w are the level-0 size; h_l = h_{l-1}/2 (floor). */
int cp_label_pyramid(const uint8_t* labels0, int batch, int h, int w, uint8_t* const* labels /*[4]*/,
                     float* const* pnorm /*[4]*/, uint8_t* const* sel /*[3]*/, void* stream);

/* ------------------------------------------------------------------------------------
 * Keypoint voting
 * ---------------------------------------------------------------------------------- */

/* CoordLSVotingWeighted.calc (casapose/pose_estimation/voting_layers_2d.py:83-122):
 * per (image, object, keypoint) fp64 sums of w(I-nn^T) and w(I-nn^T)c over the object's
 * pixels, then the 2x2 pseudo-inverse solve.  `field` is the network output
 * [n,h,w,ld] with seg logits at channel seg_off (classes = objects+1 values), directions
 * (dy,dx)*kp at dir_off and confidence logits at conf_off.  If `labels` is non-NULL it is
 * used as the hard object map instead of the arg-max of the logits (this is how the
 * connected-component filter of :43-79 is applied).  sums_ws: fp64 [n][objects][kp][5]
 * workspace (zeroed by the call).  keypoints: fp32 [n][objects][kp][2] in (y,x) pixels. */
int cp_ls_vote_f32(const float* field, int ld, int seg_off, int dir_off, int conf_off, const uint8_t* labels,
                   int batch, int h, int w, int objects, int kp, double* sums_ws, float* keypoints,
                   void* stream);
/* the same with the pixel weight selectable: sigmoid_weights = 0 -> softplus(conf) (cp_ls_vote_f32), 1 -> sigmoid(conf)
 * (CoordLSVotingWeighted(sigmoid_weights=True), voting_layers_2d.py:32-33; sigmoid_scale is 1 in the reference) */
int cp_ls_vote_w_f32(const float* field, int ld, int seg_off, int dir_off, int conf_off, const uint8_t* labels,
                     int batch, int h, int w, int objects, int kp, int sigmoid_weights, double* sums_ws, float* keypoints,
                     void* stream);
size_t cp_ls_vote_workspace_bytes(int batch, int objects, int kp);

/* Largest-connected-component filter of voting_layers_2d.py:43-79 (tfa.image.connected_components,
 * 4-connectivity, keep the largest component of each object if it has >= min_size pixels):
 * labels_in uint8 [n,h,w] -> labels_out (pixels outside the kept component become 0).
 * rank 1 = the reference's default: the histogram entry that ranks SECOND in top_k order (the first is assumed to be bin 0, "everything
 * else"); rank 2 = output_second_largest_component (:58-59,71-73: three bins, the THIRD entry).  ws: int32 workspace of cp_ccl_workspace_bytes;
 * it needs no initialisation.  A label value above `objects` is background: it joins no component, has no histogram and gives 0 in labels_out. */
int cp_ccl_filter_labels(const uint8_t* labels_in, int batch, int h, int w, int objects, int min_size, int rank, void* ws,
                         uint8_t* labels_out, void* stream);
size_t cp_ccl_workspace_bytes(int batch, int h, int w, int objects);

/* Where cp_ccl_filter_labels keeps its intermediate products inside the caller's workspace (for tests and diagnostics).  Host only; the same
 * carving the filter itself applies.  offsets[5] receives the byte offsets, from a 64-byte aligned workspace base (a base that is not is rounded
 * up to the next 64-byte boundary by the filter; cp_ccl_workspace_bytes includes that slack), of
 *   [0] parent  int32  [n*h*w]           after the call, for every pixel with a label in 1..objects: the image-global raster index
 *                                        (n*h*w + y*w + x) of the first pixel in raster order of its component; -1 for background
 *   [1] count   int32  [n*h*w]           count[r] = the component's size at root indices r only (r = a value of parent); other entries unspecified
 *   [2] roots   int32  [n][h*w]          roots[n*h*w + 0 .. nroots[n]): the roots of image n, in any order; the rest unspecified
 *   [3] nroots  int32  [n]               the number of components of image n (all objects together); 64-byte aligned
 *   [4] stats   uint64 [n][objects][3]   slot 2: the selected histogram entry of (image, object) as (thresholded count << 32) | tie, where the
 *                                        thresholded count is 0 below min_size, tie = 0xFFFFFFFF for bin 0 ("every pixel that is not the object") and
 *                                        0xFFFFFFFE - (root - n*h*w) for a component; 0 when the histogram has no such entry (fewer than rank + 1
 *                                        bins; the reference pads with empty bins there and keeps nothing).  An object without pixels has the
 *                                        one-entry histogram {bin 0 = h*w}: its slot 2 is 0 for either rank.  Slots 0 and 1 are not written.
 *                                        64-byte aligned
 * in this order, without overlap, the last one ending inside cp_ccl_workspace_bytes.  Returns -1 for a null pointer or sizes
 * cp_ccl_filter_labels refuses. */
int cp_ccl_workspace_layout(int batch, int h, int w, int objects, size_t* offsets /*[5]*/);

/* ransac_voting_layer_all_masks (casapose/pose_estimation/ransac_voting.py:276-368,447-484).
 * One call votes all (image, object) pairs.  labels: uint8 [n,h,w] hard object map
 * (arg-max one-hot of pose_evaluation.py:37-38); vertex: [n,h,w,ld] with (dy,dx)*kp at
 * dir_off.  idx: int32 [max_iter][n][objects][hyp][kp][2] uniform random draws in
 * [0, 2^31) supplied by the caller (the reference draws tf.random.uniform per round,
 * :319-321; tests inject them); a draw d selects the (d % tn)-th pixel of the object in
 * raster order (the order of tf.where, :303-305).  Objects with fewer than min_num pixels
 * give zeros (:290-292).  The random sub-sampling of objects above max_num pixels
 * (:295-301) is the caller's job (apply it to `labels`); max_num is accepted for signature
 * parity only.  Rounds stop per object when 1-(1-r_min^2)^hyps > confidence or after
 * max_iter rounds (:340-347), decided on the device; after rounds 1, 2, 4, 8, 16 the call synchronises `stream` once to learn whether any object
 * is still voting and stops launching rounds when none is.  hyp must be a multiple of 16.
 * out: fp32 [n][objects][kp][2] in (x,y); rounds_out (optional) int32 [n][objects].
 * ws: workspace of cp_ransac_workspace_bytes. */
int cp_ransac_vote_f32(const uint8_t* labels, const float* vertex, int ld, int dir_off, int batch, int h,
                       int w, int objects, int kp, const int32_t* idx, int hyp, float inlier_thresh,
                       float confidence, int max_iter, int min_num, int max_num, void* ws, float* out,
                       int32_t* rounds_out, void* stream);
/* The same voter with the random numbers made INSIDE the library from a 64-bit seed (counter-based: equal seeds give equal results, no state):
 * the pixel-pair draws of every round, and the random thinning of objects above max_num pixels (:295-301: a pixel is kept with probability
 * max_num / count) as part of the compaction -- no draw tensor (94 MB per call at the reference's settings), no pass over the mask outside. */
int cp_ransac_vote_seeded_f32(const uint8_t* labels, const float* vertex, int ld, int dir_off, int batch, int h,
                              int w, int objects, int kp, unsigned long long seed, int hyp, float inlier_thresh,
                              float confidence, int max_iter, int min_num, int max_num, void* ws, float* out,
                              int32_t* rounds_out, void* stream);
size_t cp_ransac_workspace_bytes(int batch, int h, int w, int objects, int kp, int hyp);

/* The voter's per-(image, object) state record as it lies in the workspace (csrc/ransac_vote.hip uses this very struct). */
typedef struct cp_ransac_state {
    int tn;                 /* pixels the object votes with (after the min_num gate and the seeded entry's thinning); 0 = skipped */
    int done;               /* 1: stopping rule or max_iter reached, or skipped */
    int rounds;             /* rounds voted */
    float hyp_num;          /* hypotheses drawn so far (rounds * hyp) */
    float win_ratio[9];     /* best inlier ratio so far per keypoint */
    float win_pts[9][2];    /* the hypothesis (x, y) that reached it; (0, 0) while no hypothesis had an inlier */
} cp_ransac_state;
/* Where the voter keeps its intermediate products inside the workspace, so that each stage can be read back and checked on its own.
 * Host only; the same carving the voter itself applies.  offsets[7] receives the byte offsets, from a 256-byte aligned workspace base, of
 *   [0] rowcnt   int32  [n][objects][h]           exclusive row starts of every object's pixel list
 *   [1] pixlist  int32  [n][objects][h*w]         the first st.tn entries: the object's pixels (y*w + x) in raster order
 *   [2] st       cp_ransac_state [n][objects]
 *   [3] hyp_pts  float  [n][objects][hyp][kp][2]  the hypotheses (x, y) of the last round voted; (0, 0) where |det| <= 1e-6
 *   [4] counts   int32  [n][objects][hyp][kp]     their inlier counts
 *   [5] sums     double [n][objects][kp][5]       a00, a01, a11, b0, b1 of the refinement's normal equations over the winners' inliers
 *   [6] thr      uint32 [n][objects]              cp_ransac_vote_seeded_f32 only: a pixel is kept if its 32-bit draw is below thr
 *                                                 (0xffffffff: all kept, 0: object below min_num)
 * and *state_bytes (optional) sizeof(cp_ransac_state).  What a finished call leaves behind: st, pixlist and sums are final after any call;
 * hyp_pts and counts of an object are those of the last round it voted, so after a call with max_iter = 1 they are round 1's.  Objects that
 * are skipped (st.tn = 0) leave their hyp_pts, counts and pixlist entries unwritten. */
int cp_ransac_workspace_layout(int batch, int h, int w, int objects, int kp, int hyp, size_t* offsets /*[7]*/, size_t* state_bytes);

/* Keypoint covariances from the voting distribution (PVNet's uncertainty, about a given mean): for every (image, object) pair and keypoint v,
 * `hyp` two-ray hypotheses h_j are drawn and voted exactly as one round of the voter above draws and votes them (same compaction, same
 * hypothesis and inlier kernels), c_j = the inlier count of h_j over the pair's pixels, and
 *   wsum = sum_j c_j,    cov = sum_j c_j (h_j - mean)(h_j - mean)^T / wsum    as (sxx, sxy, syy) in px^2.
 * A hypothesis with c_j = 0 is skipped (a non-finite hypothesis has no inliers and never reaches the sum).  The centred differences are
 * accumulated in fp64 by one wave per (pair, keypoint) and reduced in a fixed order: no float atomics, two calls give the same bits; cov is
 * rounded to fp32 once.  cov = 0 and wsum = 0 for a pair without pixels, a pair below min_num (counted before any thinning), wsum = 0, or a
 * non-finite mean.  wsum saturates at 2^31 - 1.
 *   labels, vertex, ld, dir_off, batch, h, w, objects, kp, hyp, inlier_thresh, min_num, max_num: as for cp_ransac_vote_f32
 *   mean   fp32 [n][objects][kp][2]   (x, y) pixels in the voter's (x + 0.5, y + 0.5) convention: the voted keypoints of either voter
 *   draws  int32 [n][objects][hyp][kp][2]   cp_kp_cov_f32: uniform in [0, 2^31), a draw d selects pixel d % tn (max_num is then signature parity)
 *   seed   cp_kp_cov_seeded_f32: the draws come from the voter's counter-based generator under another key than the voting rounds' (seed ^ a
 *          constant, as the thinning's), and objects above max_num pixels are thinned inside the compaction with the pixel decisions cp_ransac_vote_seeded_f32
 *          makes for this seed: the covariance is taken over the pixels that voted
 *   cov    fp32 [n][objects][kp][3];   wsum  int32 [n][objects][kp]
 *   ws     cp_kp_cov_workspace_bytes(...) bytes, 256-byte aligned.  The call builds its own state records; a workspace a voting call used may be
 *          reused, its contents are not.
 * hyp must be a multiple of 16 and hyp * min(max_num, h*w) < 2^31.  cp_kp_cov_workspace_layout: offsets[4] = the byte offsets of
 *   [0] pixlist  int32 [n][objects][h*w]   [1] st  cp_ransac_state [n][objects] (tn; done = (tn == 0))
 *   [2] hyp_pts  float [n][objects][hyp][kp][2]   [3] counts  int32 [n][objects][hyp][kp]
 * as after one voting round; pairs with tn = 0 leave theirs unwritten. */
int cp_kp_cov_f32(const uint8_t* labels, const float* vertex, int ld, int dir_off, int batch, int h, int w, int objects, int kp,
                  const float* mean, const int32_t* draws, int hyp, float inlier_thresh, int min_num, int max_num, void* ws, float* cov,
                  int32_t* wsum, void* stream);
int cp_kp_cov_seeded_f32(const uint8_t* labels, const float* vertex, int ld, int dir_off, int batch, int h, int w, int objects, int kp,
                         const float* mean, unsigned long long seed, int hyp, float inlier_thresh, int min_num, int max_num, void* ws, float* cov,
                         int32_t* wsum, void* stream);
size_t cp_kp_cov_workspace_bytes(int batch, int h, int w, int objects, int kp, int hyp);
int cp_kp_cov_workspace_layout(int batch, int h, int w, int objects, int kp, int hyp, size_t* offsets /*[4]*/, size_t* state_bytes);

/* GuidedBilinearUpsampling (_normalization_layers.py:569-664; casapose_c_gcu4_bilat): mask[n,Y,X] bit j = the low-resolution label of
 * tap j in {(y,x),(y,x+1),(y+1,x),(y+1,x+1)} (zero padded bottom/right) equals labels_hi[n,Y,X]; the upsampling blends the four taps
 * with the fixed sub-pixel weights after replacing non-matching taps by the mean of the matching ones (0 if none), which is the
 * 4-tap gather out = sum_j coef_j(mask, sub-pixel) * tap_j.  h, w = LOW-resolution size for the two upsampling calls. */
int cp_guided_match_mask(const uint8_t* labels_hi, const uint8_t* labels_lo, int batch, int h_hi, int w_hi, uint8_t* mask, void* stream);
int cp_guided_bilinear_upsample_x2_f32(const float* src, const uint8_t* mask, int batch, int h, int w, int channels, float* dst, void* stream);
int cp_guided_bilinear_upsample_x2_bwd_f32(const float* dy, int ld_dy, const uint8_t* mask, int batch, int h, int w, int channels, float* dx,
                                           void* stream);

/* ------------------------------------------------------------------------------------
 * Winograd F(4x4,3x3) path for deep 3x3 / stride-1 / pad == dilation convolutions (same layers.Conv2D call sites as
 * cp_conv2d_fwd_f32; the MFMA work drops 4x).  Three launches:
 *   cp_wino_input_transform_f32 : V[p][t][c_off + c] = (B^T d B)[p] for every 6x6 patch of `src` (once per source of a
 *                                 concatenated input); V is [36][tiles_padded][ldv]
 *   cp_conv2d_fwd_f32           : 1x1 over 36*tiles_padded "pixels" with group_rows = tiles_padded,
 *                                 group_weight_stride = cout*ldk and the weights of cp_wino_pack_weights_host -> M
 *   cp_wino_output_transform_f32: Y = A^T M A + the epilogue of cp_conv2d_fwd_f32 (residual, affine / per-label table,
 *                                 activation, raw and activated stores)
 * Dilation d is exact by sub-grid decomposition (d*d independent dilation-1 problems).  cp_wino_tiles returns the tile
 * count and its padding (multiple of 128).  cp_wino_pack_weights_host writes dst[p][co][k_off + c] = (G g G^T)[p] for the
 * input channels [c_begin, c_begin+real_channels) of a HWIO kernel; dst is [36][cout][ldk] and must be zeroed first.
 * ---------------------------------------------------------------------------------- */
int cp_wino_tiles(int batch, int h, int w, int dilation, int* tiles, int* tiles_padded);
/* The grouped GEMM as a dedicated persistent kernel: M[r][n] = sum_k V[r][k] * U[r / group_rows][n][k], rows = 36*tiles_padded,
 * k % 32 == 0.  Same arithmetic as the grouped mode of cp_conv2d_fwd_f32 (which remains available); the operand stream is
 * pipelined ACROSS tiles because a tile only lives for k/32 chunks. */
int cp_wino_gemm_f32(const float* V, const float* U, float* M, int rows, int group_rows, int k, int n, void* stream);
/* OPT-IN alternative with fp32-equivalent results on the bf16 matrix pipe: every operand is split exactly into three bf16 terms and six
 * of the nine products (all but the three below 2^-24) are accumulated in fp32 (csrc/wino_gemm_split.hip).  V is the same
 * fp32 tensor (split while it is staged); the weights are pre-split ONCE into fragment-major bf16 planes by cp_wino_split_weights_f32
 * (U as for cp_wino_gemm_f32: [groups][n][k] fp32; `out` of cp_wino_split_weights_bytes(groups, n, k) bytes, caller-owned).
 * group_rows must be a multiple of 128.  Selected by CASAPOSE_WINO_GEMM=split; never the default of bench.py. */
size_t cp_wino_split_weights_bytes(int groups, int n, int k);
int cp_wino_split_weights_f32(const float* U, int groups, int n, int k, void* out, void* stream);
int cp_wino_gemm_split_f32(const float* V, const void* Usplit, float* M, int rows, int group_rows, int k, int n, void* stream);
/* planes = 3: the above.  planes = 2: hi + mid planes only (16 significand bits per operand; products hi*hi, hi*mid, mid*hi): half the MFMAs, NOT
 * fp32-equivalent -- for the bf16 conv modes (BASELINE.json configs[2]; gates 3e-2).  Same pre-split weights. */
int cp_wino_gemm_split_planes_f32(const float* V, const void* Usplit, float* M, int rows, int group_rows, int k, int n, int planes, void* stream);
/* planes = CP_PLANES_F16X2: the fp16 TWO-way split (csrc/split_f16.h): hi = rn_f16(x), lo = rn_f16(x - hi) reproduce an fp32 operand to within
 * one fp32 ulp (2^-23 worst case, 0.75 * 2^-24 rms, three operands in four exactly) and the three products hi*hi, hi*lo, lo*hi are exact in the fp32 accumulator of v_mfma_f32_32x32x16_f16 -- fp32-level
 * accuracy (measured against fp64 beside the fp32 MFMA and the exact bf16 split: tests/test_gpu_f16x2.py) with HALF the MFMAs of
 * the exact bf16 split.  fp16's range is handled by scaling: the weights are multiplied by a power of two before their split
 * (cp_f16x2_weight_scale(max |w|): max -> [2^11, 2^12), so that the low parts are normal numbers) and the kernel multiplies its accumulators by
 * c_scale = 1 / scale (exact); activations are used as they are: fp32-level for max |v| in [1, 65504]; below, the low parts
 * become subnormal (absolute 2^-25: the error degrades as 2^-25 / max |v|); above, conversions clamp at +-65504 and the error grows to 2^-12 of the
 * operand -- never inf / NaN.  The split-weight buffer has the size and layout of the three-plane one (planes 0 / 1 used). */
int cp_wino_split_weights_scaled_f32(const float* U, int groups, int n, int k, int planes, float scale, void* out, void* stream);
int cp_wino_gemm_split_scaled_f32(const float* V, const void* Usplit, float* M, int rows, int group_rows, int k, int n, int planes, float c_scale,
                                  void* stream);
int cp_wino_pack_weights_host(const float* w_hwio, int cin_total, int cout, int c_begin, int channels, int real_channels, int ldk,
                              int k_off, float* dst);
/* device version of the weight transform (training: after every optimizer step): g(ky,kx,c,o) is read at
 * w[ky'*stride_ky + kx'*stride_kx + c*stride_in + o*stride_out] with (ky',kx') = flip ? (2-ky,2-kx) : (ky,kx), so the same kernel
 * serves HWIO / IHWO masters and the flipped, transposed data-gradient kernel.  U[p][o][k_off + c], rows of ldk floats. */
int cp_wino_transform_weights_f32(const float* w, long long stride_ky, long long stride_kx, long long stride_in, long long stride_out,
                                  int flip, int channels, int cout, int ldk, int k_off, float* U, void* stream);
/* weight gradient through the Winograd planes (training): dM[p][t][c] = (A dY A^T)[p] for every 4x4 tile of dy; then
 * dU[p][o][k] = sum_t dM[p][t][o] * V[p][t][k] is cp_conv2d_wgrad_f32 in its grouped mode (group_rows = tiles_padded) and
 * cp_wino_weight_grad_f32 folds the 36 planes back: dw(ky,kx,c,o) = sum_{a,b} G[a][ky] G[b][kx] dU[a*6+b][o][k_off+c], written at
 * dw[ky*stride_ky + kx*stride_kx + c*stride_in + o*stride_out] (the master layout). */
int cp_wino_dy_transform_f32(const float* dy, int ld, int channels, int batch, int h, int w, int dilation, float* dM, void* stream);
int cp_wino_weight_grad_f32(const float* dU, int channels, int cout, int ldk, int k_off, long long stride_ky, long long stride_kx,
                            long long stride_in, long long stride_out, float* dw, int accumulate, void* stream);
/* The grouped weight-gradient GEMM of the Winograd layers on the bf16 matrix pipe (csrc/wino_wgrad_split.hip):
 *   du[g][n][k] = sum_t dm[g][t][n] * v[g][t][k]      (g < groups = 36 planes, t < rows = padded tiles, n = cout, k = cin)
 * what cp_conv2d_wgrad_f32 computes in its grouped mode with fp32 MFMAs, here as exact three-way bf16 splits (planes = 3, fp32-equivalent:
 * six exact products per fp32 product, fp32 accumulation) or with operands rounded to bf16 (planes = 1).  dm = the output of
 * cp_wino_dy_transform_f32, v = the forward's transformed input, du feeds cp_wino_weight_grad_f32.  n and k multiples of 128
 * (cp_wino_wgrad_split_applicable); du is overwritten. */
int cp_wino_wgrad_split_applicable(int groups, int rows, int n, int k);
int cp_wino_wgrad_split_f32(const float* dm, const float* v, float* du, int groups, int rows, int n, int k, int planes, void* stream);
/* The same GEMM with planes = CP_PLANES_F16X2 (round 6): both operands as fp16 pairs, three exact products per fp32 product.  dm is multiplied
 * by dm_scale and v by v_scale before the split (powers of two the caller picks so that each operand's maximum sits in [0.5, 65504 / 4]:
 * cp_wino_dy_transform_f32 and the input transforms report those maxima into the armed monitor slot), du takes 1 / (dm_scale v_scale).
 * planes 1 / 3 with factors of 1 are cp_wino_wgrad_split_f32. */
int cp_wino_wgrad_split_scaled_f32(const float* dm, const float* v, float* du, int groups, int rows, int n, int k, int planes, float dm_scale,
                                   float v_scale, void* stream);
int cp_wino_input_transform_f32(const float* src, int ld, int channels, int batch, int h, int w, int dilation, float* V, int ldv,
                                int c_off, void* stream);
int cp_wino_output_transform_f32(const float* M, int cout, int batch, int h, int w, int dilation, const float* residual, int residual_ld,
                                 const float* scale, const float* shift, const uint8_t* epi_label, int act, float* out_raw,
                                 int out_raw_ld, float* out_act, int out_act_ld, void* stream);
/* The ResNet stem (conv0: 7x7 / stride 2 / pad 3, one 4-channel source, cout 64 -- the range of the CP_TILE_STEM kernel) on the bf16 matrix
 * pipe (csrc/conv_stem_split.hip, round 4): planes = 3 exact three-way bf16 splits (fp32-equivalent), planes = 1 bf16 operands.  Same descriptor
 * as cp_conv2d_fwd_f32 (input affine on real pixels, per-channel affine + activation epilogue, raw / activated outputs).  Weights:
 * cp_conv_pack_weights_stem_split_host (HOST: HWIO / IHWO kernel -> fp32 image of the fragment stream, cp_conv_stem_split_weight_floats()
 * floats), then cp_conv_split_weights_f32(image, floats, planes, out) on the device (floats / 512 * planes * 1024 bytes). */
int cp_conv_stem_split_weight_floats(void);
int cp_conv_pack_weights_stem_split_host(const float* w_host, int layout, int real_channels, float* dst_host);
int cp_conv2d_fwd_stem_split(const cp_conv_desc* d, const void* weights_split, int planes, void* stream);
/* planes = CP_PLANES_F16X2: as cp_conv2d_fwd_split_scaled (weights from cp_conv_split_weights_scaled_f32 with the same power-of-two scale) */
int cp_conv2d_fwd_stem_split_scaled(const cp_conv_desc* desc, const void* weights_split, int planes, float w_descale, void* stream);
/* Output transform of one Winograd layer FUSED with the input transform of the next (round 4): Y = A^T M A, + residual, raw store (optional),
 * t = act(Y * scale[c] + shift[c]) (per channel; optional activated store), then V[p][t][c_off + c] = (B^T t B)[p] of the consumer -- for two
 * Winograd convolutions of the same (batch, h, w, dilation) where the consumer's only source is this activated output (the residual-unit chains
 * of resnet.py:57-113 in inference).  The activated map never goes to HBM unless out_act is given.  One block owns a whole sub-grid (the pixels
 * with equal (y mod d, x mod d)) x 32 channels (60x80 at dilation 4: 4 x 5 tiles) or x 16 channels (the 30x40 sub-grids of dilation 2);
 * cp_wino_output_input_applicable says whether a geometry fits one of the two block shapes, otherwise the two separate transforms are used. */
int cp_wino_output_input_applicable(int batch, int h, int w, int dilation, int cout);
int cp_wino_output_input_transform_f32(const float* M, int cout, int batch, int h, int w, int dilation, const float* residual, int residual_ld,
                                       const float* scale, const float* shift, int act, float* out_raw, int out_raw_ld, float* out_act,
                                       int out_act_ld, float* V, int ldv, int c_off, void* stream);
/* Training-step forms of the two transforms (round 3, fused normalisation: casapose.py:76-105 / resnet.py:78-103 are convolution ->
 * normalisation -> activation -> convolution).  _stats: also accumulates stats[c] = sum, stats[cout + c] = sum of squares (fp64; zeroed by
 * the call) of the RAW output over the real pixels = the batch statistics cp_bn_stats_f32 would compute from out_raw.  _pre: applies
 * y = act(fma(x, pre_scale[c], pre_shift[c])) (cp_affine_act_f32's expression, per channel, both NULL = identity) to every real pixel as it
 * is loaded, so the activated tensor between a normalisation layer and a Winograd layer need not be stored.  pre_scale alone (pre_shift
 * NULL, pre_act CP_ACT_NONE; round 6) = a per-channel factor only: what brings a gradient into fp16's band in front of an f16x2 GEMM. */
int cp_wino_output_transform_stats_f32(const float* M, int cout, int batch, int h, int w, int dilation, const float* residual, int residual_ld,
                                       const float* scale, const float* shift, const uint8_t* epi_label, int act, float* out_raw, int out_raw_ld,
                                       float* out_act, int out_act_ld, double* stats, void* stream);
int cp_wino_input_transform_pre_f32(const float* src, int ld, int channels, int batch, int h, int w, int dilation, float* V, int ldv, int c_off,
                                    const float* pre_scale, const float* pre_shift, int pre_act, void* stream);

/* ====================================================================================
 * TRAINING PATH (train_casapose.py:494-611: forward with training=True, compute_loss,
 * tf.GradientTape gradients, Adam).  The reference gets every gradient below from
 * TensorFlow's autodiff of the layers cited at the forward entry points; the kernels here
 * are the adjoints of those layers, written out.
 * ==================================================================================== */

/* Weight gradient of cp_conv2d_fwd_f32 (Conv2DBackpropFilter of resnet.py:85-103,249; casapose.py:71-74;
 * PartialConvolution, _normalization_layers.py:325-373):
 *   dw_packed[co][k] (+)= sum_m dy[m][co] * A[m][k]
 * with A the forward's implicit im2col matrix (same descriptor: geometry, sources, tap_label; weights, outputs
 * and epilogue fields are ignored -- for a partial convolution dy is the gradient of the un-normalised sum,
 * i.e. already multiplied by row_scale, see cp_bn_act_bwd_apply_f32) and k in the packed K order, so dw_packed has the layout
 * of cp_conv_pack_weights_host.  Sources must be CP_SRC_DIRECT without pre-affine.  Split over pixels
 * with fp32 atomics: the summation order is not fixed (results reproducible to fp32 rounding only). */
int cp_conv2d_wgrad_f32(const cp_conv_desc* desc, const float* dy, int dy_ld, float* dw_packed, int accumulate, void* stream);
/* The same product on the bf16 matrix pipe (csrc/conv_wgrad_split.hip), the backward partner of cp_conv2d_fwd_split: 3x3 / stride 1 / pad 1,
 * direct sources whose channel counts are multiples of 32 plus an optional trailing 4-channel source (the image: its columns are computed by
 * the fp32 kernel), cout a multiple of 32, tap_label as above.  planes = 3: both operands split exactly into three bf16 terms, six products per
 * fp32 product, fp32 accumulation (fp32-equivalent); planes = 1: operands rounded to bf16 (BASELINE.json configs[2]); planes = CP_PLANES_F16X2
 * (round 6): both operands as fp16 pairs, three exact products -- the caller keeps max |x| and max |dy| inside [0.5, 65504 / 4] (cp_amax_f32).  Same dw_packed layout,
 * same accumulate flag, same unfixed summation order as cp_conv2d_wgrad_f32. */
int cp_conv_wgrad_split_applicable(const cp_conv_desc* desc);
int cp_conv2d_wgrad_split(const cp_conv_desc* desc, const float* dy, int dy_ld, float* dw_packed, int accumulate, int planes, void* stream);

/* The two full-resolution 1x1 heads of the training step (pv_final_conv_segmentation / pv_final_conv_vertex, pose_models.py:546,616: 32 input
 * channels, cout <= 32) as streaming kernels (csrc/head1x1.hip; exact fp32 MFMA like cp_conv2d_fwd_f32 / cp_conv2d_wgrad_f32): w and dw are the
 * Keras kernel [32][cout] itself (no packing).  x rows: 32 channels, 16-byte aligned, ld_x % 4 == 0.  dy_row_floats = floats that may be READ in
 * each dy row starting at dy (>= cout; >= 32 enables 16-byte loads, columns >= cout are ignored).  accumulate: add to dx / dw. */
int cp_head1x1_fwd_f32(const float* x, int ld_x, long long pixels, const float* w, int cout, float* out, int ld_out, void* stream);
int cp_head1x1_dgrad_f32(const float* dy, int ld_dy, int dy_row_floats, long long pixels, const float* w, int cout, float* dx, int ld_dx,
                         int accumulate, void* stream);
int cp_head1x1_wgrad_f32(const float* x, int ld_x, const float* dy, int ld_dy, long long pixels, int cout, float* dw, int accumulate, void* stream);

/* Fused normalisation of decoder blocks 5 / 10 in the training step (round 3; casapose.py:76-105 is one Keras block -- convolution,
 * (class-adaptive) normalisation, activation -- and the heads follow it, pose_models.py:546,616).  The raw convolution output x [pixels][32]
 * stays the only stored tensor: the head's forward and weight gradient recompute y = act(fma(x, scale[l], shift[l])) (tables [classes][32],
 * labels = NULL for classes == 1, act = CP_ACT_*), and the two passes of the normalisation backward recompute the head's data gradient
 * g_y = dout W^T on the matrix pipe instead of reading a stored one: same red / chan / dx as cp_bn_act_bwd_reduce_f32 / _apply_f32 fed with
 * cp_head1x1_dgrad_f32's output.  pixels % 32 == 0; every dout row has >= 32 readable floats from `dout` on (columns >= cout ignored). */
int cp_head1x1_fwd_affine_f32(const float* x, int ld_x, long long pixels, const float* scale, const float* shift, const uint8_t* labels, int classes,
                              int act, const float* w, int cout, float* out, int ld_out, void* stream);
/* The same forward writing COMPLETE output records (round 6): out[p][0 .. prefix_n) = prefix[p][0 .. prefix_n) (dense rows another head
 * wrote: the segmentation logits), out[p][prefix_n + q] = this head's column q.  Two heads that each fill a slice of [pixels][K + V] records
 * leave every 128-byte line partly written, which costs a read-modify-write in the memory system (2.2-2.7x the time of the same bytes
 * written as whole lines); with this entry point the last head is the only writer of the records.  1 <= prefix_n <= 16,
 * ld_out >= prefix_n + cout (== for whole lines). */
int cp_head1x1_fwd_affine_record_f32(const float* x, int ld_x, long long pixels, const float* scale, const float* shift, const uint8_t* labels,
                                     int classes, int act, const float* w, int cout, const float* prefix, int ld_prefix, int prefix_n, float* out,
                                     int ld_out, void* stream);
int cp_head1x1_wgrad_affine_f32(const float* x, int ld_x, const float* scale, const float* shift, const uint8_t* labels, int classes, int act,
                                const float* dy, int ld_dy, long long pixels, int cout, float* dw, int accumulate, void* stream);
int cp_head1x1_bn_bwd_reduce_f32(const float* x, int ld_x, const float* dout, int ld_dout, int dout_row_floats, long long pixels, const float* w, int cout,
                                 const float* mean, const float* rstd, const float* gamma, const float* fwd_scale, const float* fwd_shift,
                                 const uint8_t* labels, int classes, int act, double* red, double* chan, void* stream);
int cp_head1x1_bn_bwd_apply_f32(const float* x, int ld_x, const float* dout, int ld_dout, int dout_row_floats, long long pixels, const float* w, int cout,
                                const float* mean, const float* rstd, const float* gamma, const float* fwd_scale, const float* fwd_shift,
                                const uint8_t* labels, int classes, int act, const double* chan, double global_pixels, const float* row_scale,
                                float* dx, int ld_dx, void* stream);

/* The DATA gradient needs no entry point of its own: it is cp_conv2d_fwd_f32 over dy with the kernel
 * flipped and transposed (host-side repack), pad' = dilation*(k-1) - pad, the same dilation, and, for a
 * stride-2 forward, source mode CP_SRC_ZERO_INSERT_X2.  A partial convolution keeps its tap_label (the mask
 * is symmetric) and takes row_scale-multiplied dy (see cp_bn_act_bwd_apply_f32). */

/* Batch statistics of (Sync)BatchNormalization in training mode (resnet.py:78,100,247,250,303;
 * casapose.py:77; _normalization_layers.py:108): sums[c] = sum_p x[p][c], sums[C+c] = sum_p x[p][c]^2 in
 * fp64 (zeroed by the call).  The caller all-reduces `sums` across replicas (SyncBN) and derives
 * mean / biased variance.  channels % 4 == 0, <= 1024. */
int cp_bn_stats_f32(const float* x, long long pixels, int channels, int ld, double* sums, void* stream);

/* Turn the (all-reduced) statistic sums into everything the normalisation needs, in one launch:
 * mean[c], rstd[c] = 1/sqrt(biased var + eps); gamma_full/beta_full [classes][channels] (gamma [classes][real_channels]
 * or null = 1, beta likewise = 0; padding channels get 1/0); scale = gamma*rstd, shift = beta - mean*scale (pad_one: padding
 * channels get scale 0, shift 1); moving = moving*momentum + batch*(1-momentum) when moving_mean/moving_var are given
 * (Keras BatchNormalization update with the biased batch variance).  pixels = GLOBAL sample count. */
int cp_bn_finalize_f32(const double* sums, double pixels, int channels, int real_channels, int classes, const float* gamma,
                       const float* beta, float eps, int pad_one, float momentum, float* moving_mean, float* moving_var, float* mean,
                       float* rstd, float* gamma_full, float* beta_full, float* scale, float* shift, void* stream);
/* d beta[l][c] = red[(l*C+c)*2], d gamma[l][c] = red[(l*C+c)*2+1] as fp32 over the real channels (either output may be null) */
int cp_bn_param_grads_f32(const double* red, int channels, int real_channels, int classes, float* dgamma, float* dbeta, void* stream);

/* y[p][c] = act(x[p][c]*scale[l][c] + shift[l][c]), l = labels ? labels[p] : 0 -- the normalise(+CLADE
 * modulation, _normalization_layers.py:119-139)+activation (casapose.py:98-107) step with the batch
 * statistics folded into scale/shift by the caller. */
int cp_affine_act_f32(const float* x, long long pixels, int channels, int ld_x, const float* scale, const float* shift,
                      const uint8_t* labels, int act, float* y, int ld_y, void* stream);

/* Backward of y = act(gamma[l][c]*xhat + beta[l][c]), xhat = (x-mean[c])*rstd[c] (batch statistics), pass 1:
 *   red[(l*C+c)*2 + {0,1}] = sum_p {g, g*xhat}           (g = dy*act')  -> d beta[l][c], d gamma[l][c]
 *   chan[c*2 + {0,1}]      = sum_p {g*gamma, g*gamma*xhat}                -> the two batch means of pass 2
 * (fp64, zeroed by the call; gamma/beta may be null = 1/0; classes = 1 without labels).  The caller
 * all-reduces `chan` across replicas for SyncBN.
 * fwd_scale / fwd_shift (optional, [classes][channels], both or neither): the folded tables the forward's cp_affine_act_f32 was called
 * with.  When given, act' is evaluated at the forward's own pre-activation fma(x, scale, shift) -- the branch of every ReLU / leaky pair is
 * then bit-for-bit the one the forward took, so the result is the exact gradient of the piecewise-linear function the forward evaluated
 * (recomputing gamma*xhat + beta rounds differently and flips elements that sit within an ulp of zero). */
int cp_bn_act_bwd_reduce_f32(const float* x, int ld_x, const float* dy, int ld_dy, long long pixels, int channels, int classes,
                             const float* mean, const float* rstd, const float* gamma, const float* beta, const uint8_t* labels,
                             int act, const float* fwd_scale, const float* fwd_shift, double* red, double* chan, void* stream);
/* pass 2: dx = rstd*(g*gamma - chan[c][0]/N - xhat*chan[c][1]/N) * (row_scale ? row_scale[p] : 1),
 * N = global_pixels (all replicas); accumulate != 0 adds to dx (a tensor with several consumers). */
int cp_bn_act_bwd_apply_f32(const float* x, int ld_x, const float* dy, int ld_dy, long long pixels, int channels, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, const uint8_t* labels, int act,
                            const float* fwd_scale, const float* fwd_shift, const double* chan, double global_pixels, const float* row_scale,
                            float* dx, int ld_dx, int accumulate, void* stream);

/* Adjoints of MaxPooling2D(3, strides 2) after ZeroPadding2D(1) (resnet.py:252-253), UpSampling2D(bilinear)
 * (casapose.py:135-140) and the GuidedUpsampling gather (_normalization_layers.py:554-558).  Gather form
 * (every input pixel sums the output gradients that reference it): deterministic, no atomics.
 * h, w are the LOW-resolution (input) sizes for the two upsampling adjoints. */
int cp_maxpool3x3s2_bwd_f32(const float* x, const float* dy, int batch, int h, int w, int channels, float* dx, int accumulate,
                            void* stream);
/* The training step's pair (round 3): the forward also records the arg-max TAP (0..8, raster order, first maximum wins, zero padding takes
 * part) of every output element in idx [batch][ho][wo][channels] (one byte each, 4-byte aligned), and the adjoint routes dy by those bytes
 * without reading x: same dx as cp_maxpool3x3s2_bwd_f32. */
int cp_maxpool3x3s2_idx_f32(const float* src, int batch, int h, int w, int channels, float* dst, uint8_t* idx, void* stream);
int cp_maxpool3x3s2_bwd_idx_f32(const uint8_t* idx, const float* dy, int batch, int h, int w, int channels, float* dx, int accumulate, void* stream);
int cp_upsample_bilinear_x2_bwd_f32(const float* dy, int ld_dy, int batch, int h, int w, int channels, float* dx, void* stream);
int cp_guided_upsample_x2_bwd_f32(const float* dy, int ld_dy, const uint8_t* sel, int batch, int h, int w, int channels, float* dx,
                                  void* stream);

/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0 -- re-pack the master (Keras-layout) weights into a kernel layout after
 * an optimizer step; cp_scatter_f32 is the inverse (packed weight gradient -> master layout; idx injective on
 * its non-negative entries). */
int cp_gather_f32(const float* src, const int32_t* idx, long long n, float* dst, void* stream);
int cp_scatter_f32(const float* src, const int32_t* idx, long long n, float* dst, int accumulate, void* stream);
/* out = alpha*a + beta*b (b may be null) */
int cp_axpby_f32(const float* a, float alpha, const float* b, float beta, long long n, float* out, void* stream);

/* tf.keras.optimizers.Adam.apply_gradients (train_casapose.py:334-347,611; epsilon 1e-7):
 *   g = grads*grad_scale; m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g^2;
 *   params -= lr*sqrt(1-b2^step)/(1-b1^step) * m/(sqrt(v)+eps)          (step counts from 1) */
int cp_adam_step_f32(float* params, const float* grads, float* m, float* v, long long n, float lr, float beta1, float beta2,
                     float eps, int step, float grad_scale, void* stream);
/* the same step under a device-side skip (dynamic loss scaling's skip, without a host synchronisation): skip[0] with bit 31 set -- an f16x2
 * monitor slot's overflow bit (cp_f16x2_monitor_set, word [3]) or several combined -- leaves params, m and v unchanged; otherwise the step
 * runs with the bias correction of step - skip[1] (skip[1] = steps skipped before this one, kept by the caller on the device). */
int cp_adam_step_masked_f32(float* params, const float* grads, float* m, float* v, long long n, float lr, float beta1, float beta2,
                            float eps, int step, float grad_scale, const uint32_t* skip, void* stream);

/* compute_loss for the merged-output models (train_casapose.py:40-145), value AND gradient:
 *   loss_sums[0] mask   = mean softmax cross-entropy(labels_ce)                         (:59-60)
 *   loss_sums[1] vertex = smooth_l1_loss(dirs, unit vectors to the keypoints, fg)        (loss_functions.py:14-44)
 *   loss_sums[2] proxy  = proxy_voting_loss_v2(loss_per_object=False)                    (loss_functions.py:132-203)
 * out: network output [batch,h,w,ld] = [seg_dim logits | 2*kp directions (dy,dx) | ...]; labels_ce / labels_fg:
 * uint8 [batch,h,w] (target_seg / filtered_seg as class indices); keypoints_yx: fp32 [batch][objects][kp][2].
 * With filter_with_segmentation the foreground keeps only pixels whose arg-max prediction equals labels_fg
 * (:64-69); with filter_high_proxy_errors objects whose mean smooth-L1 proxy distance (proxy_voting_dist, loss_functions.py:47-129;
 * objects with < 20 pixels count as 0) is >= 5 are dropped from it as well (:71-93).  object_loss_values (optional, [batch][objects])
 * receives those per-object values.  dout [batch*h*w][dld] receives d(mask_w*mask + vertex_w*vertex + proxy_w*proxy)/d out with the
 * logit gradients in columns [0,seg_dim) and the direction gradients in [vert_off, vert_off+2kp); every other
 * column is zeroed.  ws: cp_pose_loss_workspace_bytes. */
size_t cp_pose_loss_workspace_bytes(int batch, int h, int w);
int cp_pose_loss_f32(const float* out, int ld, int seg_dim, int kp, const uint8_t* labels_ce, const uint8_t* labels_fg,
                     const float* keypoints_yx, int objects, int batch, int h, int w, int filter_with_segmentation,
                     int filter_high_proxy_errors, float mask_w, float vertex_w, float proxy_w, void* ws, float* dout, int dld,
                     int vert_off, double* loss_sums, float* object_loss_values, void* stream);

/* Where cp_pose_loss_f32 keeps its intermediate products inside the caller's workspace (for tests and diagnostics).  Host only; the same
 * carving the loss itself applies.  offsets[5] receives the byte offsets, from the workspace pointer, of
 *   [0] fg      uint8  [batch*h*w]        the foreground label map the vertex / proxy terms used: labels_fg after the segmentation filter and,
 *                                         with filter_high_proxy_errors, after the removal of the flagged objects
 *   [1] count   int32  [batch]            foreground pixels of each image in that map
 *   [2] objsum  double [batch*objects]    per (image, object), index b*objects + o: the smooth-L1 proxy distances summed over the object's
 *                                         pixels and keypoints, on the segmentation-filtered map
 *   [3] objcnt  int32  [batch*objects]    the object's pixels in that map
 *   [4] bad     uint8  [batch*objects]    1 where the reported value (0 below 20 pixels, else objsum / (kp*objcnt + 1e-3)) is not < 5
 * in this order, without overlap, the last one ending inside cp_pose_loss_workspace_bytes.  [2]..[4] are written only when
 * filter_high_proxy_errors or object_loss_values is given; each has room for 64 objects per image.  Returns -1 for a null pointer or a
 * shape cp_pose_loss_f32 refuses. */
int cp_pose_loss_workspace_layout(int batch, int h, int w, size_t* offsets /*[5]*/);

/* cp_pose_loss_f32 for SEVERAL INSTANCES of one object per image (the reference's max_count > 1: compute_vertex_hcoords_batch_v3,
 * image_utils.py:17-63; the instance axis of proxy_voting_loss_v2 / proxy_voting_dist, loss_functions.py:47-203).  Everything as
 * cp_pose_loss_f32 -- the cross-entropy, the two filters, the normalisations, the gradient row, loss_sums, object_loss_values, the workspace
 * and its five products -- except:
 *   keypoints_yx  fp32 [batch][objects][instances][kp][2], instances in 1..16
 *   inst_counts   int32 [batch][objects], required; entry n in 0..instances (the caller checks the range): only instances r < n of the object
 *                 exist, entries at r >= n are never read into a result (they may hold anything, NaN included)
 *   inst_map      uint8 [batch][h][w] or null: the 0-based instance of its object that owns the pixel
 * A foreground pixel of an object with n == 0, or with inst_map[p] >= n, leaves the foreground before anything is counted: fg = 0, not in
 * count, not in the object sums, no vertex or proxy term.
 * inst_map == null, the reference's rule: the vertex target is the unit vector to the keypoints of the instance whose keypoint 0 is nearest
 * to the pixel centre (first minimum over r < n); the proxy distance of keypoint j is the minimum over r < n of |v_y a_x - v_x a_y| / |v|
 * (first minimum, independently per keypoint), its gradient goes through that instance, and the per-object sums use the same minimum.
 * inst_map given, the exact rule: both terms use instance inst_map[p].
 * With instances == 1, every count 1 and no map the maps, counts, object products and dout are cp_pose_loss_f32's byte for byte.
 * Refused before any launch: a null inst_counts, instances outside 1..16, and whatever cp_pose_loss_f32 refuses.
 * cp_pose_loss_inst_workspace_bytes / _layout: the size and the five offsets of cp_pose_loss_workspace_bytes / _layout. */
size_t cp_pose_loss_inst_workspace_bytes(int batch, int h, int w);
int cp_pose_loss_inst_workspace_layout(int batch, int h, int w, size_t* offsets /*[5]*/);
int cp_pose_loss_inst_f32(const float* out, int ld, int seg_dim, int kp, const uint8_t* labels_ce, const uint8_t* labels_fg,
                          const float* keypoints_yx, int objects, int instances, const int32_t* inst_counts, const uint8_t* inst_map,
                          int batch, int h, int w, int filter_with_segmentation, int filter_high_proxy_errors, float mask_w, float vertex_w,
                          float proxy_w, void* ws, float* dout, int dld, int vert_off, double* loss_sums, float* object_loss_values,
                          void* stream);

/* compute_loss for the `pvnet` model with SEPARATED vector fields (train_casapose.py:57,97-125): the output holds seg_dim logits followed by
 * objects*2*kp direction channels, object o in [seg_dim + o*2kp, seg_dim + (o+1)*2kp).  vertex = sum over objects of smooth_l1_loss(slice,
 * target slice, one-hot of the object), proxy = sum over objects of proxy_voting_loss_v2(slice, the object's keypoints, one-hot of the object):
 * a pixel contributes to the slice of its own object only, normalised by 2kp * (pixels of that object in the image) + 1e-3, mean over the
 * batch.  Everything else as cp_pose_loss_f32 (labels, filter_with_segmentation, the gradient row: logits in [0,seg_dim), the directions of
 * object o in [vert_off + o*2kp, ...)).  ws: cp_pose_loss_sep_workspace_bytes. */
size_t cp_pose_loss_sep_workspace_bytes(int batch, int h, int w, int seg_dim);
int cp_pose_loss_sep_f32(const float* out, int ld, int seg_dim, int kp, const uint8_t* labels_ce, const uint8_t* labels_fg,
                         const float* keypoints_yx, int objects, int batch, int h, int w, int filter_with_segmentation, float mask_w,
                         float vertex_w, float proxy_w, void* ws, float* dout, int dld, int vert_off, double* loss_sums, void* stream);

/* The same for cp_pose_loss_sep_f32.  offsets[2]: [0] fg uint8 [batch*h*w], labels_fg after the segmentation filter; [1] counts int32
 * [batch][seg_dim], the pixels of label l of image b in that map at b*seg_dim + l (entry 0 of an image stays 0).  Host only. */
int cp_pose_loss_sep_workspace_layout(int batch, int h, int w, int seg_dim, size_t* offsets /*[2]*/);

/* The reference's loss / target functions as stand-alone passes (values only; the training step differentiates the fused kernels above).
 * They back the importable casapose.utils.loss_functions / casapose.utils.image_utils modules.
 *
 * cp_vector_field_f32 -- compute_vertex_hcoords_batch_v3 (utils/image_utils.py:17-63) and, with separated != 0, the per-object concatenation of
 * get_all_vectorfields (:66-79): out[p][slot*2kp + 2j..] = (keypoint_j - pixel centre) of the pixel's object (label l in 1..objects, slot =
 * separated ? l-1 : 0), l2-normalised when normalize != 0 (tf.math.l2_normalize, epsilon 1e-12), zero elsewhere.  keypoints_yx:
 * [batch][objects][instances][kp][2]; with several instances the one whose first keypoint (the centre) is nearest to the pixel is used. */
int cp_vector_field_f32(const uint8_t* labels, const float* keypoints_yx, int batch, int h, int w, int objects, int instances, int kp,
                        int separated, int normalize, float* out, int ld, void* stream);
/* smooth_l1_loss (utils/loss_functions.py:14-44) up to its final normalisation: sums[2b] = sum over the image's pixels and channels of
 * smoothL1(|w (pred - target)|), sums[2b+1] = sum of w; w = weights[p*wld] (wmode 0), |1 - weights[p*wld]| (wmode 1, `invert_weights`) or 1
 * (wmode 2, `ignore_weights`).  elem (optional, [batch*pixels][channels]) receives the per-element values (`normalize=False, reduce=False`). */
int cp_smooth_l1_f32(const float* pred, int pld, const float* target, int tld, const float* weights, int wld, int wmode, int channels,
                     int batch, long long pixels_per_image, double* sums, float* elem, void* stream);
/* proxy_voting_dist / proxy_voting_loss_v2 (utils/loss_functions.py:47-203) up to their final normalisations: per pixel and keypoint the
 * perpendicular distance between the keypoint of the pixel's object (labels: 0 = no object -> object 0, as the arg-max of an all-zero one-hot
 * row; l -> object l-1; minimum over the object's instances) and the line through the pixel centre along the predicted direction, times the
 * pixel weight (as cp_smooth_l1_f32).  img_sums[2b], [2b+1] = sum of smoothL1(dist), sum of weights; obj_sums / obj_counts (optional,
 * [batch][objects]) = the same sum per object (unsorted_segment_sum) and the object's pixel count; dist_out / elem (optional, [pixels][kp]) =
 * the distances / their smooth-L1 values. */
int cp_proxy_voting_f32(const float* pred, int pld, int kp, const uint8_t* labels, const float* weights, int wld, int wmode,
                        const float* keypoints_yx, int objects, int instances, int batch, int h, int w, double* img_sums, double* obj_sums,
                        int32_t* obj_counts, float* dist_out, float* elem, void* stream);

/* Backward of cp_ls_vote_f32 (the reference differentiates CoordLSVotingWeighted with tf.GradientTape,
 * train_casapose.py:555-579): dkeypoints = d loss / d keypoints [batch][objects][kp][2] (y,x px); sums_ws = the workspace
 * the forward left behind; pu_ws: float [batch*objects*kp*4] scratch.  Writes (accumulate: adds) d loss / d directions
 * into dfield[pix][ddir_off + 2j..] and d loss / d confidence logits into dfield[pix][dconf_off + j] for the pixels of
 * each object (zero elsewhere).  Optionally adds conf_coef[b][j]*sigmoid(conf) on the pixels with reg_labels != 0 (the
 * confidence regulariser of keypoint_reprojection_loss, loss_functions.py:254-262).  `labels` is required. */
int cp_ls_vote_bwd_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* labels, int batch, int h, int w,
                       int objects, int kp, const double* sums_ws, const float* dkeypoints, float* pu_ws,
                       const uint8_t* reg_labels, const float* conf_coef, float* dfield, int dld, int ddir_off, int dconf_off,
                       int accumulate, void* stream);
/* counts[0][b][c] / counts[1][b][c] = pixels of class c in labels / labels_est (may be null) of image b; conf_sums[b][j] =
 * sum over labels != 0 of softplus(conf_j) (fp64) -- objects_available and the confidence regulariser
 * (loss_functions.py:236-262).  Zeroed by the call. */
int cp_kp_stats_f32(const float* field, int ld, int conf_off, const uint8_t* labels, const uint8_t* labels_est, int batch, int h, int w,
                    int classes, int kp, int32_t* counts, double* conf_sums, void* stream);
/* keypoint_reprojection_loss without BPnP (loss_functions.py:207-344): coords_yx [batch*objects][kp][2] voted keypoints
 * (crop pixels), affine [batch][6] row-major 2x3 crop->image map of transform_points_back_tf_batch, gt_xy the projected
 * ground-truth keypoints (image pixels), avail [batch*objects] in {0,1}.  loss = sum_n avail*mean_j cap(smoothL1(|gt - T(p)|))
 * / sum(avail); g_yx = weight * d loss / d coords_yx. */
int cp_kp_reproj_loss_f32(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, int batch, int objects,
                          int kp, float max_pixel_error, float weight, float* g_yx, double* loss_out, void* stream);

/* ---- input pipeline: training batches assembled on the device (csrc/augment.hip) -----------------------------------------------
 * One cp_aug_image per image, filled by the host (casapose_amd/data_handler/augment.py) and copied to the device with the batch; every
 * kernel below reads the program of image b from progs[b] and handles the whole batch in one launch, on the caller's stream, with no
 * allocation, synchronous copy or synchronisation.  Added in ABI 302 without changing any earlier struct or entry point. */
#define CP_AUG_MAX_OPS 12
#define CP_AUG_MAX_LUTS 6
#define CP_AUG_MAX_TAPS 49          /* 7 x 7: the widest linear blur of the imgaug sequence */
#define CP_AUG_NOISE_MAX 16         /* side of the largest FrequencyNoise field */
#define CP_AUG_NOISE_FIELDS 3       /* iterations of its IterativeNoiseAggregator */
#define CP_AUG_FINISH_SLOT 15       /* Philox counter slot of the Gaussian noise of cp_aug_finish */

/* op kinds of the photometric program (cp_aug_photometric); the Philox counter of a random op is (slot, pixel, channel, 0) */
enum cp_aug_op_kind {
    CP_AUG_LUT = 1,          /* out[c] = lut[c][in[c]]: Add, Multiply, Gamma / Sigmoid / Log / Linear contrast (host-built, already rounded) */
    CP_AUG_HUE_SAT = 2,      /* RGB -> HSV (OpenCV 8-bit) ; h = (h + i0) mod 180 ; s = clip(s + i1) ; HSV -> RGB */
    CP_AUG_FREQ_BLEND = 3,   /* a = noise mask ; out = round(a lut[i0](x) + (1 - a) lut[i1](x)) */
    CP_AUG_GAUSS_NOISE = 4,  /* out = round(clip(x + N(0, f0))) */
    CP_AUG_LAPLACE_NOISE = 5,/* out = round(clip(x + Laplace(0, f0))) */
    CP_AUG_POISSON_NOISE = 6,/* out = clip(x +- Poisson(f0)), sign uniform */
    CP_AUG_DROPOUT = 7,      /* out = 0 with probability f0 */
    CP_AUG_REPLACE = 8,      /* with probability f0: out = round(255 r), r = Beta(.5,.5) folded by i0 (0 both, 1 salt, 2 pepper) */
    CP_AUG_BLUR_LINEAR = 9,  /* correlation with the k x k taps[i0] (anchor k/2), reflect-101 border */
    CP_AUG_BLUR_MEDIAN = 10, /* k x k median (k odd), replicate border */
    CP_AUG_BLUR_BILATERAL = 11 /* OpenCV bilateral: radius k, f0 = sigma colour, f1 = sigma space, reflect-101 border */
};

typedef struct cp_aug_op {
    int32_t kind;            /* cp_aug_op_kind */
    int32_t per_channel;     /* random ops: 1 = one draw per channel, 0 = one per pixel shared by the channels */
    int32_t slot;            /* Philox counter slot */
    int32_t k;               /* blur window (linear / median: side; bilateral: radius) */
    int32_t i0, i1;          /* integer parameters (see the kinds) */
    float f0, f1;            /* real parameters (see the kinds) */
} cp_aug_op;

typedef struct cp_aug_image {
    uint64_t seed;                   /* Philox key of the image */
    int64_t src_offset;              /* pixel offset of the image in the source buffers: rgb at 3 * src_offset, segmentation at src_offset */
    int32_t src_h, src_w;            /* decoded size */
    int32_t crop_x, crop_y;          /* crop origin in the (warped) source */
    int32_t warp;                    /* 0: plain crop; 1: affine warp first (PIL AFFINE, output -> input map `affine`, fill 0) */
    int32_t n_ops;                   /* photometric ops in `ops` (blur kinds contiguous, at most two) */
    double affine[6];                /* x_in = a0 x + a1 y + a2, y_in = a3 x + a4 y + a5 at output pixel centres (x + .5, y + .5) */
    float brightness;                /* cp_aug_finish: added to the 0..255 image (0 = off) */
    float contrast;                  /* cp_aug_finish: (v - mean) * contrast + mean per channel (1 = off; needs channel sums) */
    float noise_sigma;               /* cp_aug_finish: Gaussian noise of the normalised image (0 = off) */
    int32_t noise_fields;            /* CP_AUG_FREQ_BLEND: fields aggregated (1..3) */
    int32_t noise_h[CP_AUG_NOISE_FIELDS], noise_w[CP_AUG_NOISE_FIELDS], noise_up[CP_AUG_NOISE_FIELDS];  /* size, upscale 0 nearest 1 linear 2 cubic */
    int32_t noise_aggregate;         /* 0 max, 1 average */
    int32_t noise_sigmoid;           /* 1: a = 1 / (1 + exp(-(20 a - 10 - noise_threshold))) */
    float noise_threshold;
    cp_aug_op ops[CP_AUG_MAX_OPS];
    float taps[2][CP_AUG_MAX_TAPS];  /* linear blur weights, row-major k x k */
    float noise[CP_AUG_NOISE_FIELDS][CP_AUG_NOISE_MAX * CP_AUG_NOISE_MAX];  /* FrequencyNoise fields in [0,1], row-major h x w */
    uint8_t label_map[256];          /* segmentation id -> training label (0 = background) */
    uint8_t lut[CP_AUG_MAX_LUTS][3][256];
} cp_aug_image;

size_t cp_aug_image_size(void);
/* A: warp + crop.  src_rgb uint8 HWC, src_seg uint8 HW (all images of the batch, at progs[b].src_offset); crop_rgb [batch][crop_h][crop_w][3]
 * (bilinear, PIL's rounding) and crop_lab [batch][crop_h][crop_w] (nearest, then label_map). */
int cp_aug_geometry(const uint8_t* src_rgb, const uint8_t* src_seg, const cp_aug_image* progs, int batch, int crop_h, int crop_w,
                    uint8_t* crop_rgb, uint8_t* crop_lab, void* stream);
/* B: the photometric program of every image on uint8 [batch][h][w][3] (in != out).  Pointwise ops before the blurs run while a tile and its
 * halo are loaded to LDS, then up to two blurs, then the remaining ops; uint8 rounding after every op.  tile_hint 0: 32 x 32 tiles, 1: 16 x 8
 * (same result). */
int cp_aug_photometric(const uint8_t* in, const cp_aug_image* progs, int batch, int h, int w, int tile_hint, uint8_t* out, void* stream);
/* C1: PIL BILINEAR resize of uint8 rgb [batch][in_h][in_w][3] and NEAREST resize of labels to out_h x out_w (in != out). */
int cp_aug_resize(const uint8_t* in_rgb, const uint8_t* in_lab, int batch, int in_h, int in_w, int out_h, int out_w, uint8_t* out_rgb,
                  uint8_t* out_lab, void* stream);
/* C2: sums[b][c] = sum of channel c of image b (uint32, zeroed by the call with an asynchronous memset on `stream`). */
int cp_aug_channel_sums(const uint8_t* rgb, int batch, long long pixels, uint32_t* sums, void* stream);
/* C3: img fp32 [batch][h][w][3] = clip(((brightness / contrast of rgb) / 255 - .5) / .5 + N(0, noise_sigma), -1, 1); filtered int32
 * [batch][h][w] = labels; target fp32 [batch][h][w][classes] = one-hot of labels.  sums may be null when no image has contrast != 1. */
int cp_aug_finish(const uint8_t* rgb, const uint8_t* lab, const cp_aug_image* progs, const uint32_t* sums, int batch, int h, int w,
                  int classes, float* img, int32_t* filtered, float* target, void* stream);

/* ---- input pipeline: inference frames (csrc/frames.hip) ------------------------------------------------------------------------
 * Network input from decoded uint8 frames, the per-pixel half of ImageOnlyDataset.load_images (image_only_dataset.py:36-49; host side in
 * casapose_amd/data_handler/image_only_dataset.py).  src: [batch][h][w][channels] uint8 with channels 1, 3 or 4, rows `src_pitch` bytes
 * apart (>= w * channels), images `src_stride` bytes apart (>= h * src_pitch).  out: fp32 [batch][h][w][3] (dense),
 * out = ((float)v / 255.0f - norm0) / norm1 with IEEE fp32 divisions (bit-identical to NumPy's float32 formula); one channel is replicated
 * to three, a fourth (alpha) is dropped.  At most 2^30 pixels per call.  Added in ABI 302 without changing any earlier entry point. */
int cp_frames_to_input_f32(const uint8_t* src, int batch, int h, int w, int channels, long long src_pitch, long long src_stride,
                           float norm0, float norm1, float* out, void* stream);

/* ---- pose statistics (csrc/pose_eval.hip) ----------------------------------------------------------------------------------------
 * The per-(image, object) record of map_estimates (ransac_voting.py:561-625); evaluate_poses (:627-687) is the sum of the records over the
 * batch.  Everything is device memory and fp32 unless noted.
 *   points     [objects][vmax][3]  evaluation meshes; rows counts[o] .. vmax-1 are never read
 *   counts     int32 [objects]     vertices per mesh.  The library cannot see it: counts[o] > vmax is the caller's error and is clamped to vmax
 *                                  in the kernel (negative values to 0); an empty mesh gives NaN means, like a mean of nothing
 *   symmetric  int32 [objects]     non-zero selects ADD-S (nearest estimated point, brute force) instead of ADD
 *   pairs      [batch*objects][36] one record per pair, pair = image * objects + object: estimated pose (12, row-major 3x4), ground-truth
 *                                  pose (12), camera matrix K (9, row-major), diameter, valid flag (object is in the ground truth), one pad
 *   records    [batch*objects][6]  (err_2d, err_3d, valid_3d, valid_2d, missing, false_positive):
 *                                  valid == 0: zeros but false_positive = |sum of the pose| > 1e-4;  valid != 0 and |sum| < 1e-4:
 *                                  (99.9, 999.9, 0, 0, 1, 0);  else the mean 2-D reprojection distance (pixel = 0 where the projective z is
 *                                  exactly 0), the mean ADD or ADD-S distance (ADD-S per point: sqrt(|min_j d^2| + 1e-5)),
 *                                  err_3d < 0.1 * diameter and err_2d < allowed_error_2d
 *   point_err2, point_err3         optional [batch*objects][vmax] (NULL in production): the 2-D distance and the ADD / ADD-S distance of target
 *                                  point i; 0 for skipped pairs and for i >= counts[o]
 *   workspace                      cp_pose_eval_workspace_bytes(batch, objects, vmax) bytes, 8-byte aligned (0 for non-positive arguments)
 * fp32 arithmetic on direct coordinate differences, fp64 sums in a fixed order without atomics: two calls on the same input give bit-identical
 * records.  At most 65535 pairs per call, vmax <= 2^24.  cp_pose_eval_est_tile(): the number of estimated points one LDS tile of the ADD-S walk
 * holds (tests place their sizes by it).  Added in ABI 302 without changing any earlier entry point. */
size_t cp_pose_eval_workspace_bytes(int batch, int objects, int vmax);
int cp_pose_eval_est_tile(void);
int cp_pose_eval_f32(const float* points, const int32_t* counts, const int32_t* symmetric, int objects, int vmax, const float* pairs, int batch,
                     float allowed_error_2d, void* workspace, float* records, float* point_err2, float* point_err3, void* stream);

/* ---- pose statistics for several instances per object (csrc/pose_match.hip, csrc/match_math.h, csrc/pose_eval_math.h) ------------------------
 * For every group = (image b, object o): up to `slots` estimated poses against up to `instances` ground-truth instances.  Every (estimate e,
 * instance g) pair gets the two mean errors of cp_pose_eval_f32 -- the same per-point arithmetic and the same order of summation
 * (pose_eval_math.h), so a finite entry of `err` equals records 0 and 1 of cp_pose_eval_f32 on that pair bit for bit -- and the pairs are
 * matched greedily by the 3-D error: repeatedly the smallest finite cost among the free non-empty estimates and the free instances g < count,
 * on ties the smaller g, then the smaller e (match_math.h).  No distance gates a match: a far match is simply no true positive.  Everything is
 * device memory and fp32 unless noted.
 *   points, counts, symmetric, objects, vmax   the evaluation meshes, exactly as cp_pose_eval_f32 takes them
 *   est        [batch][objects][slots][12]      estimated poses, row-major 3x4.  A slot whose |sum of the 12 entries| < 1e-4 is empty, as
 *                                               cp_pose_eval_f32 decides a zero pose
 *   gt         [batch][objects][instances][12]  ground-truth poses; rows at and beyond the group's count are never read
 *   gt_counts  int32 [batch][objects]           instances per group, read as clamped to [0, instances]
 *   cams       [batch][9]                       K per image, row-major
 *   diameters  [objects]
 *   err        [batch][objects][slots][instances][2]  (err_2d, err_3d): the mean 2-D reprojection distance and the mean ADD, or ADD-S where
 *                                               symmetric[o] is set; (+inf, +inf) for an empty estimate and for g >= count
 *   gt_rec     [batch][objects][instances][5]   (matched slot or -1, err_2d, err_3d, valid_3d = err_3d < 0.1 * diameter, valid_2d = err_2d <
 *                                               allowed_error_2d) of the match, compared in fp64; (-1, 0, 0, 0, 0) for an instance without a
 *                                               match and for g >= count
 *   est_match  int32 [batch][objects][slots]    the matched g; -1 for a non-empty estimate without a match (a false positive); -2 for an
 *                                               empty slot
 *   tally      int32 [batch][objects][5]        (ground-truth instances, non-empty estimates, matched, valid_3d matches, valid_2d matches)
 *   workspace  cp_pose_match_workspace_bytes(batch, objects, vmax, slots, instances) bytes, 8-byte aligned (0 for arguments the call refuses);
 *              needs no initialisation
 * A cost that is not finite (an empty mesh gives NaN means) is never matched.  fp64 sums in a fixed order without atomics: two calls on the
 * same input give the same bytes.  slots and instances in 1..16, batch * objects * slots <= 65535, vmax <= 2^24.  Added in ABI 302 without
 * changing any earlier entry point. */
size_t cp_pose_match_workspace_bytes(int batch, int objects, int vmax, int slots, int instances);
int cp_pose_match_f32(const float* points, const int32_t* counts, const int32_t* symmetric, int objects, int vmax, const float* est, int slots,
                      const float* gt, int instances, const int32_t* gt_counts, const float* cams, const float* diameters, int batch,
                      float allowed_error_2d, void* workspace, float* err, float* gt_rec, int32_t* est_match, int32_t* tally, void* stream);

/* ---- BOP pose errors with object symmetries (csrc/bop_errors.hip, csrc/bop_math.h) -------------------------------------------------------
 * For every pair of an estimated pose P^ and a ground-truth pose P_ of one object, over the object's symmetry transforms S and the vertices x of
 * its evaluation mesh:  e_MSSD = min_S max_x |P^ x - P_ S x| (millimetres),  e_MSPD = min_S max_x |proj_K(P^ x) - proj_K(P_ S x)| (pixels), with
 * the projection of cp_pose_eval_f32 (a general 3x3 K, pixel 0 where the projective z is exactly 0).  Everything is device memory and fp32 unless
 * noted.
 *   points        [objects][vmax][3]  evaluation meshes; rows counts[o] .. vmax-1 are never read
 *   counts        int32 [objects]     vertices per mesh, clamped to [0, vmax] in the kernel; an object without vertices gives +inf
 *   syms          [objects][smax][12] symmetry transforms, row-major 3x4 [R|t], the identity included by the caller; rows sym_counts[o] ..
 *                                     smax-1 are never read
 *   sym_counts    int32 [objects]     transforms per object, clamped to [0, smax]
 *   pairs         [npairs][36]        the record of cp_pose_eval_f32: estimated pose (12, row-major 3x4), ground-truth pose (12), K (9,
 *                                     row-major); the last three floats are not read
 *   object_index  int32 [npairs]      the object of each pair; an index outside [0, objects) gives +inf
 *   errors        [npairs][2]         (e_MSSD, e_MSPD).  (+inf, +inf) where the estimate is the zero pose: |sum of its 12 entries| < 1e-4, as
 *                                     cp_pose_eval_f32 decides it, or a sum that is not finite
 *   per_symmetry  optional [npairs][smax][2] (NULL in production): the two maxima under every symmetry; +inf at and beyond sym_counts[o] and for
 *                                     pairs whose errors are +inf
 *   workspace     cp_bop_errors_workspace_bytes(npairs, smax) bytes, 8-byte aligned (0 for non-positive arguments)
 * P_ S is composed once per (pair, symmetry) in fp64 and rounded once to fp32; distances are direct coordinate differences; the maximum is taken
 * over squared distances with one root per (pair, symmetry).  No atomics: two calls on the same input give bit-identical output.  vmax <= 2^24,
 * smax <= 2^16, npairs * ceil(smax / cp_bop_errors_sym_group()) < 2^24 per call.  cp_bop_errors_tile(): the vertices a block takes per step;
 * cp_bop_errors_sym_group(): the symmetries a block takes (tests place their sizes by both).  Added in ABI 302 without changing any earlier entry
 * point. */
size_t cp_bop_errors_workspace_bytes(int npairs, int smax);
int cp_bop_errors_tile(void);
int cp_bop_errors_sym_group(void);
int cp_bop_errors_f32(const float* points, const int32_t* counts, int objects, int vmax, const float* syms, const int32_t* sym_counts, int smax,
                      const float* pairs, const int32_t* object_index, int npairs, void* workspace, float* errors, float* per_symmetry,
                      void* stream);

/* ---- device PnP (csrc/pnp.hip, csrc/pnp_math.h) -----------------------------------------------------------------------------------
 * Voted keypoints -> [3,4] poses for every (image, object) pair of a batch: casapose_amd/pose_estimation/pnp.py restated in fp64.  One block per
 * pair, one thread per hypothesis: EPnP on a 5-point set, inliers at <= reprojection_error over all n points; the consensus is the hypothesis
 * with the most inliers, then the smallest sum of squared inlier errors, then the lowest index (no atomics: two calls give the same bits).  Then
 * EPnP on the consensus set (on all points when it has fewer than 5), Levenberg-Marquardt over all n points, (rvec, t) rounded to fp32, and the
 * pose negated when t_z < 0.  pair = image * oc + object; everything is device memory for cp_pnp_f64 and host memory for cp_pnp_host_f64.
 *   points_xy  fp32 [b*oc][n][2]   keypoints (x, y), crop pixels when `affine` is given, image pixels otherwise
 *   points_3d  fp32 [b*oc][n][3]   model keypoints
 *   K          fp32 [b][9] (k_per_image != 0) or [9] shared by all images (k_per_image == 0), row-major
 *   affine     fp64 [b][6] or NULL: image x = a0 x + a1 y + a2, image y = a3 x + a4 y + a5 (what transform_points_back computes from `offsets`)
 *   solve      int32 [b*oc]        0: write the zero pose and status 1 without reading the pair's points
 *   table      uint8 [H][5]        the hypotheses: point indices < n (a row that names another point is a hypothesis without a pose)
 *   poses      fp32 [b*oc][12]     row-major [3,4]
 *   info       int32 [b*oc][4]     status, winning hypothesis, its inlier count, LM iterations.  Status: 0 solved; 1 not asked for (solve == 0);
 *                                  2 a non-finite input; 3 degenerate (all 2-D points coincide, or the 3-D points lie on one line); 4 no finite
 *                                  solution.  Every status but 0 comes with the zero pose, winner -1 and zeros.
 *   cost       fp32 [b*oc][2]      the all-point squared reprojection error before and after LM
 * 5 <= n <= 16, 1 <= H <= 256, at most 65535 pairs per call.  Every loop has a fixed trip count (30 Jacobi sweeps, 10 Gauss-Newton steps, 20 LM
 * iterations of 10 damping tries).  cp_pnp_host_f64 runs the same code serially and launches nothing: it works without a GPU.  A hypothesis
 * is not comparable with pnp.py's (the null space of a 5-point system has dimension >= 2 and the eigen-solvers return different bases of it);
 * the final pose is the same local optimum.  Added in ABI 302 without changing any earlier entry point. */
int cp_pnp_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine, const int32_t* solve,
               const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, float* poses, int32_t* info, float* cost, void* stream);
int cp_pnp_host_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine, const int32_t* solve,
                    const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, float* poses, int32_t* info, float* cost);
/* Uncertainty-weighted PnP (csrc/pnp_weighted.hip): cp_pnp_f64 whose final LM minimises the Mahalanobis reprojection error.  The consensus stage and both EPnP calls
 * are cp_pnp_f64's (plain pixel errors against reprojection_error); only the LM over all points differs, with the same damping schedule, trip
 * counts and relative stop.
 *   cov        fp32 [b*oc][n][3]   (sxx, sxy, syy) per keypoint in the pixel system of points_xy (cp_kp_cov_f32's output); never NULL -- callers
 *                                  without covariances use cp_pnp_f64
 *   cov_floor  added to sxx and syy before anything else (>= 0, finite)
 *   weighted   int32 [b*oc]        1: solved with weights; 0: not solved (status != 0), or solved exactly as cp_pnp_f64 solves it
 * Per point Sigma = cov + cov_floor I, with an affine Sigma' = M Sigma M^T for M = [[a0, a1], [a3, a4]], Sigma' = L L^T (lower Cholesky), and the
 * residual (ru, rv) with its two Jacobian rows becomes ru' = ru / l00, rv' = (rv - l10 ru') / l11.  If any point of a pair has a non-finite
 * Sigma' or one without positive pivots, the whole pair takes cp_pnp_f64's path and weighted = 0.  cost: the Mahalanobis cost before and after
 * LM when weighted = 1.  Added in ABI 302 without changing any earlier entry point. */
int cp_pnp_weighted_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine, const int32_t* solve,
                        const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, const float* cov, float cov_floor, float* poses,
                        int32_t* info, float* cost, int32_t* weighted, void* stream);
int cp_pnp_weighted_host_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine,
                             const int32_t* solve, const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, const float* cov,
                             float cov_floor, float* poses, int32_t* info, float* cost, int32_t* weighted);

/* ---- BPnP keypoint loss (csrc/bpnp.hip, csrc/bpnp_math.h) ----------------------------------------------------------------------------
 * keypoint_reprojection_loss with use_bpnp_reprojection_loss = 1 (loss_functions.py:264-323) and its gradient, on the device:
 * training.bpnp_reprojection_loss_host restated in fp64.  Per available (image, object) pair: the voted keypoints go through the crop->image
 * affine, the consensus EPnP + LM of cp_pnp_f64 gives the pose (before its fp32 rounding), a second LM (30 iterations, relative stop 1e-14)
 * tightens it to the optimum y; r = project(points_3d, y), e = (|r - p'| + |gt - r|) / 2, smooth L1 with the soft cap at max_pixel_error, the
 * mean over the keypoints.  The gradient is the explicit term plus the implicit-function term through the PnP optimum: H v = J^T g_r with
 * H = d(J^T r)/dy by central differences (h = 1e-6 max(1, |y_k|), symmetrised), then g_direct + J v, back through the 2x2 linear part of the
 * affine, as (y, x).  Two launches on `stream` (one block per pair, then one block), no atomics: two calls give the same bits.
 *   coords_yx  fp32 [batch*objects][kp][2]  voted keypoints (y, x) in crop pixels
 *   gt_xy      fp32 [batch*objects][kp][2]  projected ground-truth keypoints (x, y) in image pixels
 *   affine     fp32 [batch][6]              image x = a0 x + a1 y + a2, image y = a3 x + a4 y + a5 (as for cp_kp_reproj_loss_f32)
 *   avail      fp32 [batch*objects]         0: the pair takes no part (status 1, zero gradient, zero pose)
 *   points_3d  fp32 [batch*objects][kp][3]  model keypoints
 *   K          fp32 [9]                     one camera for the whole batch, row-major (the reference uses camera_data[0])
 *   table      uint8 [H][5]                 the hypotheses of cp_pnp_f64
 *   g_yx       fp32 [batch*objects][kp][2]  weight x d loss / d coords_yx; every element is written
 *   loss_out   fp64 [1]                     sum of the solved pairs' losses / their number na; 0 when na == 0
 *   poses      fp32 [batch*objects][12]     row-major [3,4] of the tightened optimum, negated when t_z < 0; zero for every pair that is not solved
 *   info       int32 [batch*objects][4]     cp_pnp_f64's words: status, winning hypothesis, its inlier count, iterations of the first LM.  Status 4
 *                                           also covers a singular H or a non-finite loss
 *   counts     int32 [2]                    {solved pairs (na), available pairs that are not solved}
 *   workspace  cp_bpnp_loss_workspace_bytes(batch, objects, kp) bytes, 8-byte aligned; needs no initialisation
 * A pair is solved when avail != 0 and its status is 0.  An available pair that is not solved (a collapsed vote, a non-finite keypoint, no finite
 * optimum) is treated as unavailable: no loss, no gradient, not in na -- where the host path raises FloatingPointError for the whole step.
 * 5 <= kp <= 16, 1 <= H <= 256, at most 65535 pairs per call, reprojection_error > 0, max_pixel_error > 0.  cp_bpnp_loss_host_f64 runs the same
 * code serially on host pointers, launches nothing and also checks that the table names points below kp.  Added in ABI 302 without changing
 * any earlier entry point. */
size_t cp_bpnp_loss_workspace_bytes(int batch, int objects, int kp);
int cp_bpnp_loss_f64(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, const float* points_3d, const float* K,
                     const uint8_t* table, int batch, int objects, int kp, int H, float reprojection_error, float max_pixel_error, float weight,
                     float* g_yx, double* loss_out, float* poses, int32_t* info, int32_t* counts, void* workspace, void* stream);
int cp_bpnp_loss_host_f64(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, const float* points_3d, const float* K,
                          const uint8_t* table, int batch, int objects, int kp, int H, float reprojection_error, float max_pixel_error, float weight,
                          float* g_yx, double* loss_out, float* poses, int32_t* info, int32_t* counts, void* workspace);

/* ---- synthetic scenes (csrc/scenes.hip, csrc/scene_math.h) ------------------------------------------------------------------------------
 * SyntheticSceneDataset._render (data_handler/synthetic_scene.py) on the device: ray-cast ellipsoids, the background wave, the noise, the label
 * map, the one-hot target and the visible-pixel counts of b images in one launch.  All geometry is fp64 without FMA contraction; the image is
 * rounded to fp32 once.
 *   records    fp64 [b][cp_render_scenes_record_words(oc)]  one record per image, built on the host: words 0-1 the crop origin (row hc, column
 *              wc), 2-5 the camera fx, fy, cx, cy, 6 the image seed (the bit pattern of a uint64), 7 the number of objects in this image
 *              (0..oc; anything else renders the background alone), then per object R [9] row-major, t [3], 1 / semi-axes [3], colour [3]
 *   noise      0: the noise-free image; otherwise N(0, 0.02) per channel on background pixels, then N(0, 0.01) per channel everywhere, from
 *              Philox4x32-10 keyed by the image seed and counted by (pixel, draw), Box-Muller in fp32: the six normals of a pixel depend on
 *              (image seed, pixel) alone, not on the batch, the position in it or the launch shape
 *   img        fp32 [b][H][W][3] in [-1, 1]
 *   label      uint8 [b][H][W]    0 the background, o + 1 object o (the nearest hit; index order with a strict <)
 *   target_seg fp32 [b][H][W][oc + 1]  one-hot of label
 *   counts     int32 [b][oc]      visible pixels per object; zeroed inside the call, integer atomics only
 * 1 <= oc <= 254, 1 <= b <= 65535, H * W < 2^31; records 8-byte aligned, img / target_seg / counts 4-byte aligned.  Widths that are a multiple
 * of 4 with 16-byte aligned img / target_seg and 4-byte aligned label take 16-byte stores; every other case stores element by element.  No
 * floating-point atomics: two calls with the same records give the same bits.  cp_render_scenes_host_f32 runs the same code serially on host
 * pointers and launches nothing: it works without a GPU.  Added in ABI 302 without changing any earlier entry point. */
size_t cp_render_scenes_record_words(int oc);
int cp_render_scenes_f32(const double* records, int b, int oc, int H, int W, int noise, float* img, uint8_t* label, float* target_seg,
                         int32_t* counts, void* stream);
int cp_render_scenes_host_f32(const double* records, int b, int oc, int H, int W, int noise, float* img, uint8_t* label, float* target_seg,
                              int32_t* counts);

/* Scenes with several instances of one object (csrc/slot_labels.hip): cp_render_scenes_f32 is given objects * instances slots, slot
 * o * instances + r being instance r of object o (an absent instance's record placed behind the camera), so its label map is the slot map
 * `o * instances + r + 1`, 0 on background.  This pass turns slots uint8 [batch][pixels_per_image] into label uint8 (the class
 * (slot - 1) / instances + 1), instance_seg uint8 ((slot - 1) % instances; both 0 on background and for a slot above objects * instances),
 * target_seg fp32 [batch][pixels_per_image][objects + 1] (the one-hot of the class) and counts int32 [batch][objects] (pixels of each class).
 * instances in 1..16, objects * instances <= 254.  Integer atomics only: the same bits on every run. */
int cp_slot_labels_u8(const uint8_t* slots, int batch, int objects, int instances, long long pixels_per_image, uint8_t* label,
                      uint8_t* instance_seg, float* target_seg, int32_t* counts, void* stream);

/* ---- segmentation masks of BOP frames (csrc/masks.hip, csrc/mask_math.h) ----------------------------------------------------------------
 * The compute step of the dataset converter (data_handler/bop_converter.py, the reference's create_ndds_mask): every instance's mesh
 * rasterised at its ground-truth pose with a z-buffer, each pixel labelled with its nearest instance, for a batch of frames.
 *   verts        fp32 [objects][Vmax][3]   vert_counts int32 [objects]   the meshes; an object uses its first vert_counts vertices
 *   faces        int32 [objects][Tmax][3]  face_counts int32 [objects]   triangles as indices into the object's vertices
 *   cams         fp64 [frames][4]          fx, fy, cx, cy
 *   inst_counts  int32 [frames]            instances of the frame, clamped to [0, instances_max]
 *   inst_obj     int32 [frames][instances_max]      object index     inst_label int32 [frames][instances_max]  label 0..255
 *   poses        fp64 [frames][instances_max][12]   row-major [3,4] model -> camera
 *   label        uint8 [frames][H][W]      the label of the nearest instance (lowest index on an exact fp32 tie), 0 where nothing was hit
 *   records      int32 [frames][instances_max][11]  px_count_all, px_count_visib, bbox_obj (x, y, w, h), bbox_visib (x, y, w, h),
 *                dropped_triangles; w = xmax - xmin, h = ymax - ymin (the BOP toolkit's boxes), (-1, -1, -1, -1) for an empty pixel set;
 *                slots at or above the frame's instance count hold an empty record
 *   workspace    cp_render_masks_workspace_bytes(frames, instances_max, H, W) bytes, 4-byte aligned: one uint32 depth plane per
 *                (frame, instance); needs no initialisation
 * The arithmetic is fixed (camera points and depths in fp64 without contraction, vertices snapped to 1/256 pixel, exact int64 edge functions,
 * closed edges, both windings; pixel (i, j) sampled at (j + sample_offset, i + sample_offset)) and listed in csrc/mask_math.h.  A triangle with a
 * vertex at Z < near, with a face index outside its object's vertices or projecting beyond 2^20 pixels is dropped whole and counted in
 * dropped_triangles; an instance whose object index or label is out of range renders nothing.  Integer atomics only: two calls with the same
 * inputs give the same bytes.  1 <= frames <= 65535, 1 <= instances_max <= 256, H, W <= 16384, 0 < near <= far, 0 <= sample_offset <= 1.
 * cp_render_masks_workspace_bytes returns 0 for sizes outside these limits.  After the call plane [frame][instance] of the workspace holds,
 * per pixel, the bit pattern of the instance's own nearest fp32 depth (whether or not another instance occludes it there) or 0xffffffff where
 * the instance was not hit; cp_vsd_counts_i32 reads the planes and the records' bbox_obj.  cp_render_masks_host_u8 runs the same code serially
 * on host pointers and launches nothing: it works without a GPU.  Added in ABI 302 without changing any earlier entry point. */
size_t cp_render_masks_workspace_bytes(int frames, int instances_max, int H, int W);
int cp_render_masks_u8(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                       int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                       const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                       uint8_t* label, int32_t* records, void* workspace, size_t workspace_bytes, void* stream);
int cp_render_masks_host_u8(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                            int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                            const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                            uint8_t* label, int32_t* records, void* workspace, size_t workspace_bytes);

/* ---- shaded pictures of meshes (csrc/shade.hip, csrc/shade_math.h) ---------------------------------------------------------------------
 * cp_render_masks_u8's geometry with a colour output: the image source of `--data meshes:<folder>` (data_handler/mesh_scene.py).  The meshes,
 * cameras, instance tables, poses, near / far / sample_offset are that entry point's arguments and follow its rules (csrc/mask_math.h rules
 * 1-6); what is added:
 *   colors       uint8 [objects][Vmax][3]  per-vertex colours, or null: every object then takes its flat colour
 *   flat_colors  fp32 [objects][3]         in [0, 1]
 *   lights       fp64 [frames][8]          the unit light direction in camera space (3), ambient, diffuse, the noise seed (the bit pattern of
 *                                          a uint64), crop row and crop column (where the procedural background is taken)
 *   background   uint8 [frames][H][W][3]   or null: scene_math.h's wave at the frame's crop origin
 *   noise        0: the noise-free image; otherwise N(0, 0.02) per channel on background pixels, then N(0, 0.01) per channel everywhere, the
 *                Philox words of cp_render_scenes_f32 keyed by the frame's seed and counted by pixel
 *   img          fp32 [frames][H][W][3] in [-1, 1]: clip(albedo * (ambient + diffuse * max(0, n . l)), 0, 1) * 2 - 1 with the albedo
 *                interpolated perspective-correctly from the winning triangle's vertex colours and n its flat two-sided face normal
 *   label        uint8 [frames][H][W]      inst_label of the winning instance, 0 on background: byte for byte cp_render_masks_u8's label
 *   depth        fp32 [frames][H][W] or null: the winning fp32 depth, 0 on background
 *   dropped      int32 [frames]            triangles dropped at the near plane or for an index out of range, over the frame's instances
 *   workspace    cp_render_shaded_workspace_bytes(frames, H, W) = 8 bytes per pixel and frame, 8-byte aligned; cleared by the call.  After it
 *                the workspace holds per pixel depth_bits << 32 | instance << 24 | triangle of the winner, all ones where nothing was hit
 * One key per pixel decides visibility: the smallest depth, then the lowest instance index, then the lowest triangle index, so every output
 * is independent of the order of arrival.  Integer atomics only: two calls with the same inputs give the same bytes.  1 <= frames <= 65535,
 * instances_max <= 256, Tmax <= 2^24, H, W <= 16384, 0 < near <= far; cp_render_shaded_workspace_bytes returns 0 outside these limits.  Widths
 * that are a multiple of 4 with 16-byte aligned img / depth and 4-byte aligned label take 16-byte stores; every other case stores element by
 * element.  The rules are listed in csrc/shade_math.h.  cp_render_shaded_host_f32 runs the same code serially on host pointers and launches
 * nothing: it works without a GPU.  Added in ABI 302 without changing any earlier entry point. */
size_t cp_render_shaded_workspace_bytes(int frames, int H, int W);
int cp_render_shaded_f32(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                         int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                         const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                         const uint8_t* colors, const float* flat_colors, const double* lights, const uint8_t* background, int noise, float* img,
                         uint8_t* label, float* depth, int32_t* dropped, void* workspace, size_t workspace_bytes, void* stream);
int cp_render_shaded_host_f32(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                              int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                              const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                              const uint8_t* colors, const float* flat_colors, const double* lights, const uint8_t* background, int noise,
                              float* img, uint8_t* label, float* depth, int32_t* dropped, void* workspace, size_t workspace_bytes);

/* ---- BOP's Visible Surface Discrepancy (csrc/vsd.hip, csrc/vsd_math.h) -------------------------------------------------------------------
 * For every pair of a rendered estimate and a rendered ground-truth instance of one image, the integers BOP's VSD error is made of: the pixels
 * of the visible union, of the visible intersection and, per tau, the intersection pixels whose cost |d_g - d_e| / diameter reaches tau (BOP19
 * visibility with tolerance delta against the sensor's depth image; distances from the camera centre in fp64; the rules are listed in
 * csrc/vsd_math.h).  The error e_k = (counts[2 + k] + counts[0] - counts[1]) / counts[0] is the caller's (pose_estimation/bop_vsd.py).
 * Everything is device memory.
 *   planes     uint32 [nplanes][H][W]   the workspace of cp_render_masks_u8 after the call, nplanes = frames * instances_max
 *   records    int32 [nplanes][11]      its records; words 2-5 (bbox_obj: x, y, w, h) bound the pixels a plane is read at
 *   depth      fp32 [images][H][W]      sensor depth in millimetres; a value that is not > 0 (0, negative, NaN) is missing
 *   cams       fp64 [images][4]         fx, fy, cx, cy; pixel centres at integer coordinates
 *   pairs      int32 [npairs][4]        (image, estimate plane, ground-truth plane, unused)
 *   diameters  fp64 [npairs]            the object's diameter, which normalises the cost
 *   taus       fp64 [ntau]              1 <= ntau <= 32, in any order
 *   split      blocks per pair, 1 .. 64: a speed setting, the counts do not depend on it
 *   counts     int32 [npairs][2 + ntau] zeroed inside the call: union, intersection, then one count per tau
 * A pair walks the union of its two planes' boxes clipped to the image and nothing else.  A pair whose image or plane index is out of range,
 * whose diameter is not > 0 or whose two boxes are empty leaves zeros.  Integer atomics only: two calls with the same inputs give the same
 * bytes.  H, W <= 16384, npairs * split < 2^31, delta >= 0.  cp_vsd_tile(): the pixels a block takes per step (tests place their sizes by it).
 * There is no host twin: the arithmetic's host coverage is csrc/vsd_selftest.cpp.  Added in ABI 302 without changing any earlier entry point. */
int cp_vsd_tile(void);
int cp_vsd_counts_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams, int images,
                      const int32_t* pairs, const double* diameters, int npairs, double delta, const double* taus, int ntau, int split,
                      int32_t* counts, void* stream);

/* ---- depth refinement: projective point-to-plane ICP (csrc/depth_icp.hip, csrc/icp_math.h) -----------------------------------------------
 * One Gauss-Newton step per job = (image, rendered plane, gate): every pixel of the plane's bbox_obj, clipped to [1, W-2] x [1, H-2], whose
 * rendered depth z and four neighbours are hit without a depth step of jump x gate or more and whose sensor depth d has d > 0 and |d - z| < gate
 * gives a normal n from the central differences of the back-projected plane, a residual r = n . (q - p) and a Jacobian J = (p x n, n); the
 * sums of J J^T, J r and r r are solved with relative damping by Cholesky for xi = (omega, v), and the pose becomes dR R, dR t + v with dR
 * the rotation of the unit quaternion (1, omega / 2) / |.| (the rules are listed in csrc/icp_math.h).  Everything is device memory.
 *   planes     uint32 [nplanes][H][W]   the workspace of cp_render_masks_u8 after the call, nplanes = frames * instances_max
 *   records    int32 [nplanes][11]      its records; words 2-5 (bbox_obj: x, y, w, h) bound the pixels a plane is read at
 *   depth      fp32 [images][H][W]      sensor depth in millimetres; a value that is not > 0 (0, negative, NaN) is missing
 *   cams       fp64 [images][4]         fx, fy, cx, cy; pixel centres at integer coordinates
 *   jobs       int32 [njobs][4]         (image, plane, unused, unused); with update = 1 no two jobs may name the same plane
 *   gates      fp64 [njobs]             millimetres, > 0
 *   jump       in gates, > 0            damping >= 0: times diag(A)         min_pixels >= 1
 *   update     1: rewrite the poses of the jobs that solved; 0: stats and status only
 *   split      blocks per job in the accumulation, 1 .. 64: a speed setting, no bit of the result depends on it
 *   poses      fp64 [nplanes][12]       the poses the planes were rendered at -- the renderer's own `poses` argument -- rewritten in place,
 *                                       so the next cp_render_masks_u8 on the same stream renders the refined poses
 *   stats      fp64 [njobs][4]          pixels used, RMS residual before the update, |omega|, |v|
 *   status     int32 [njobs]            0 solved; 1 fewer than min_pixels pixels; 2 a Cholesky pivot was not positive; 3 the job was
 *                                       refused: image or plane index out of range or gate not > 0 (nothing is read for it, stats are zeros).
 *                                       Every status but 0 leaves the pose as it is
 *   workspace  cp_depth_icp_workspace_bytes(njobs, H, W) bytes, 8-byte aligned: per job one record of 29 fp64 words (28 sums, the count)
 *              per tile of cp_depth_icp_tile() pixels of the largest clipped box; needs no initialisation
 * The order of summation is fixed (lane sums, one 64-lane tree per tile, tiles in index order) and there are no floating-point atomics: two
 * calls with the same inputs, any split and any workspace contents give the same bytes.  No pixel outside the clipped box grown by one pixel
 * is addressed.  H, W <= 16384, njobs * split < 2^31.  cp_depth_icp_workspace_bytes returns 0 for sizes outside these limits.
 * cp_depth_icp_step_host_f64 runs the same code serially on host pointers and launches nothing: it works without a GPU and gives the
 * device's bytes.  Added in ABI 302 without changing any earlier entry point. */
int cp_depth_icp_tile(void);
size_t cp_depth_icp_workspace_bytes(int njobs, int H, int W);
int cp_depth_icp_step_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                          int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels, int update,
                          int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int cp_depth_icp_step_host_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                               int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels,
                               int update, int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- mask refinement: contour alignment against a label map (csrc/mask_contour.hip, csrc/contour_math.h) ---------------------------------
 * cp_mask_edt_u16: per job = (image, label) the exact squared Euclidean distance, clamped just past the gate, to the object's trusted boundary.
 * A seed is a pixel of the label with a 4-neighbour inside the image whose label is 0; a neighbour of another label (an occlusion edge) or
 * outside the image makes no seed.  D2(p) = min(min over seeds |p - s|^2, gate^2 + 1); without seeds gate^2 + 1 everywhere.
 *   labels     uint8 [images][H][W]     the filtered label map (cp_ccl_filter_labels), 0 = background
 *   jobs       int32 [njobs][2]         (image, label)
 *   gate       whole pixels, 1 .. 255
 *   planes     uint16 [njobs][H][W]     every word of every accepted job's plane is written: needs no initialisation
 *   status     int32 [njobs]            0 done; 3 refused: image outside [0, images) or label outside [1, 255] (nothing of the job's plane or
 *                                       workspace is written)
 *   workspace  cp_mask_edt_workspace_bytes(njobs, H, W) bytes, 2-byte aligned (the row pass: uint16 [njobs][H][W]); needs no initialisation
 * Integers only and no atomics: the planes do not depend on the workspace's contents.  H, W <= 16384; cp_mask_edt_workspace_bytes returns 0
 * outside these limits or where njobs x H x ceil(W / 256) or njobs x ceil(H / 32) x ceil(W / 64) blocks are more than 2^31 - 1.
 * cp_contour_step_f64: one Gauss-Newton step per job = (image, rendered plane, field plane, gate) on the rendered silhouette.  A pixel of the
 * plane's bbox_obj clipped to [1, W-2] x [1, H-2] is a contour pixel when it is hit and one of its four neighbours is not; it is used when its
 * depth is > 0 and D2 at it and its four neighbours is <= gate^2.  e = ((D2(x+1,y) - D2(x-1,y)) / 4, (D2(x,y+1) - D2(x,y-1)) / 4), J = the
 * projection's Jacobian at the back-projected pixel times [-[p]x | I]; A += (J^T e)(e^T J) / (e . e), b -= J^T e; the solve and the pose update are
 * cp_depth_icp_step_f64's (the rules are listed in csrc/contour_math.h).  Everything is device memory.
 *   planes, records, nplanes, cams, poses, damping, min_pixels, update, split   as cp_depth_icp_step_f64
 *   fields     uint16 [nfields][H][W]   planes of cp_mask_edt_u16
 *   sample_offset  the `sample_offset` the planes were rendered with, 0 .. 1: pixel (x, y) is back-projected from (x + o, y + o), o in whole
 *                  256ths of a pixel as the rasteriser rounds it
 *   jobs       int32 [njobs][4]         (image, plane, field, gate in pixels); with update = 1 no two jobs may name the same plane
 *   stats      fp64 [njobs][4]          used pixels, RMS of |e| in pixels before the update, contour pixels, sum e . e
 *   status     int32 [njobs]            0 solved; 1 fewer than min_pixels used pixels; 2 a Cholesky pivot was not positive; 3 refused: image,
 *                                       plane or field index out of range or gate outside [1, 255] (nothing is read for it, stats are zeros).
 *                                       Every status but 0 leaves the pose as it is
 *   workspace  cp_contour_step_workspace_bytes(njobs, H, W) bytes, 8-byte aligned: per job one record of 30 fp64 words (28 sums, two counts)
 *              per tile of cp_contour_tile() pixels of the largest clipped box; needs no initialisation
 * The order of summation is cp_depth_icp_step_f64's and there are no atomics: two calls with the same inputs, any split and any workspace
 * contents give the same bytes.  The host twins run the same code serially on host pointers and launch nothing: they work without a GPU and
 * give the device's bytes.  Added in ABI 302 without changing any earlier entry point. */
int cp_contour_tile(void);
size_t cp_mask_edt_workspace_bytes(int njobs, int H, int W);
size_t cp_contour_step_workspace_bytes(int njobs, int H, int W);
int cp_mask_edt_u16(const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int gate, uint16_t* planes, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);
int cp_mask_edt_host_u16(const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int gate, uint16_t* planes, int32_t* status,
                         void* workspace, size_t workspace_bytes);
int cp_contour_step_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const uint16_t* fields, int nfields,
                        const double* cams, int images, const int32_t* jobs, int njobs, double sample_offset, double damping, int min_pixels, int update,
                        int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int cp_contour_step_host_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const uint16_t* fields, int nfields,
                             const double* cams, int images, const int32_t* jobs, int njobs, double sample_offset, double damping, int min_pixels,
                             int update, int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- pose verification: a rendered estimate against the label map and the vector field (csrc/pose_verify.hip, csrc/verify_math.h) ---------
 * Per job = (image, rendered plane, label) the integers a score is made of.  Nothing but `counts` and the workspace is written: the entry
 * point reads another kernel's output and rewrites none of it.  Everything is device memory.
 *   planes       uint32 [nplanes][H][W]   the workspace of cp_render_masks_u8 after the call
 *   records      int32 [nplanes][11]      its records; words 2-5 (bbox_obj: x, y, w, h) bound the pixels a plane is read at
 *   inst_counts  int32 [frames]           the renderer's own, read as clamped to [0, instances_max].  Plane p is slot p % instances_max of
 *                                         frame p / instances_max; the planes that may hide it are the first inst_counts[frame] of that frame
 *   labels       uint8 [images][H][W]     the filtered label map or the slot map, 0 = background
 *   field        fp32 [images][H][W][ld]  keypoint k's direction is (dy, dx) at words dir_off + 2k, dir_off + 2k + 1 of a pixel's record, as
 *                                         in csrc/ls_vote.hip: the production record is ld 36 / dir_off 9 / kp 9; 1 <= kp <= 32,
 *                                         2 <= ld <= 4096, 0 <= dir_off, dir_off + 2 kp <= ld
 *   kp2d         fp64 [njobs][kp][2]      the job's keypoints projected by its pose, (y, x) in pixels of the label map's frame
 *   jobs         int32 [njobs][4]         (image, plane, label 1..255, unused); several jobs may name one plane
 *   sample_offset  0 .. 1: pixel (i, j) has its centre at (i + sample_offset, j + sample_offset)
 *   cos_min      0 .. 1: the smallest cosine between a direction and the ray to the keypoint that makes an inlier
 *   split        blocks per job, 1 .. 64: a speed setting, the counts do not depend on it
 *   counts       int32 [njobs][8], zeroed inside the call.  Words 0-4 walk the job's bbox_obj clipped to the image:
 *                  0 rendered       pixels where the job's own plane is hit (its word is not 0xffffffff)
 *                  1 hidden         of those, pixels where another plane q of the frame has a smaller word, or an equal word and q < p (depths
 *                                   are positive fp32: comparing the words compares the depths); q is read inside its own bbox_obj only
 *                  2 on_label       visible pixels (rendered, not hidden) whose label is the job's
 *                  3 on_background  visible pixels with label 0
 *                  4 on_other       visible pixels with any other label: reported, and neutral in pose_estimation/pose_verify.py's score
 *                  5 label_pixels   pixels of the whole image whose label is the job's
 *                  6 pairs          over on_label pixels, the (pixel, keypoint) pairs whose direction d has d.d > 0 and finite and whose
 *                                   e = kp2d - centre has e.e > 0 and finite
 *                  7 inliers        of those, the pairs with d.e >= 0 and (d.e)^2 >= cos_min^2 (d.d) (e.e)
 *   workspace    cp_pose_verify_workspace_bytes(images) bytes, 4-byte aligned: the label histogram int32 [images][256] of the same call;
 *                needs no initialisation
 * Words 6-7 are fp64 from the fp32 inputs, one rounding per operation, without contraction, square root or division (the rules are listed in
 * csrc/verify_math.h).  A job whose image, plane or label is out of range, or whose frame is not below `frames`, leaves zeros.  Integer
 * atomics only: two calls with the same inputs, any split and any workspace contents give the same bytes.  No pixel outside a clipped box is
 * addressed but by the histogram.  H, W <= 16384, H x W x kp < 2^31, instances_max <= 256, images <= 2^22, njobs * split < 2^31;
 * cp_pose_verify_workspace_bytes returns 0 outside its limit.  cp_pose_verify_tile(): the pixels a block takes per step (tests place their
 * sizes by it).  cp_pose_verify_host_i32 runs the same code serially on host pointers and launches nothing: it works without a GPU and gives
 * the device's bytes.  Added in ABI 302 without changing any earlier entry point. */
int cp_pose_verify_tile(void);
size_t cp_pose_verify_workspace_bytes(int images);
int cp_pose_verify_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                       int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp, const double* kp2d,
                       const int32_t* jobs, int njobs, double sample_offset, double cos_min, int split, int32_t* counts, void* workspace,
                       size_t workspace_bytes, void* stream);
int cp_pose_verify_host_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                            int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp,
                            const double* kp2d, const int32_t* jobs, int njobs, double sample_offset, double cos_min, int split, int32_t* counts,
                            void* workspace, size_t workspace_bytes);

/* ---- keypoints and models_info of a mesh set (csrc/models.hip, csrc/model_math.h) --------------------------------------------------------
 * What the dataset converter needs per object and BOP archives do not hold (data_handler/model_prep.py): the axis-aligned box, the squared
 * diameter (the largest squared distance over all vertex pairs) and no_points keypoints, the box centre followed by farthest-point samples of
 * the vertices, for all objects of a model folder in one call.
 *   verts        fp32 [total][3]           the vertices of all objects, back to back
 *   offsets      int64 [objects]           first vertex of each object        counts  int32 [objects]  its vertex count N
 *   diameter_sq  fp64 [objects]            max over pairs of (dx*dx + dy*dy) + dz*dz, differences, products and sums in fp64 without FMA
 *   box          fp32 [objects][6]         min x, y, z, max x, y, z
 *   keypoints    fp32 [objects][no_points][3]   keypoint 0 = 0.5 * ((double)min + (double)max) rounded to fp32; keypoint k >= 1 = the vertex
 *                farthest from the centre and the earlier picks (largest minimum squared distance, lowest index among equals), unchanged
 *   indices      int32 [objects][no_points - 1] the picked vertices' indices within their object
 *   status       int32 [objects]           CP_MODEL_OK; CP_MODEL_BAD_COUNT: N outside [1, 2^22] or the vertex range outside [0, total) -- every
 *                output of the object is zero and none of its vertices is read; CP_MODEL_TOO_FEW_DISTINCT: fewer distinct vertices than
 *                keypoints -- the picks that could not be made are zero, box and diameter are valid
 *   workspace    cp_model_prep_workspace_bytes(objects, total) bytes, 8-byte aligned; needs no initialisation
 * 1 <= objects <= 1024, 2 <= no_points <= 32 (it counts the centre), 0 <= total <= 2^32; cp_model_prep_workspace_bytes returns 0 outside these
 * limits.  Memory beyond an object's own N is never treated as a point.  Maxima and lowest-index arg-maxima only: two calls with the same inputs
 * give the same bits.  cp_model_prep_host_f32 runs the same code serially on host pointers and launches nothing: it works without a GPU.
 * Added in ABI 302 without changing any earlier entry point. */
#define CP_MODEL_OK 0
#define CP_MODEL_BAD_COUNT 1
#define CP_MODEL_TOO_FEW_DISTINCT 2
size_t cp_model_prep_workspace_bytes(int objects, long long total);
int cp_model_prep_f32(const float* verts, long long total, const long long* offsets, const int32_t* counts, int objects, int no_points,
                      double* diameter_sq, float* box, float* keypoints, int32_t* indices, int32_t* status, void* workspace,
                      size_t workspace_bytes, void* stream);
int cp_model_prep_host_f32(const float* verts, long long total, const long long* offsets, const int32_t* counts, int objects, int no_points,
                           double* diameter_sq, float* box, float* keypoints, int32_t* indices, int32_t* status, void* workspace,
                           size_t workspace_bytes);

/* ---- several instances of one object per image (csrc/ccl.hip, csrc/ls_vote.hip) -----------------------------------------------------------
 * The reference's voter (casapose/pose_estimation/voting_layers_2d.py:43-122) keeps ONE component per (image, object) and has one row of sums
 * per object.  These entry points extend both to R = max_instances instances: the vector field is shared by all classes and the label map
 * says which pixel votes for what, so a label map whose values name (object, instance) pairs -- a slot map -- is all the voter needs.
 *
 * THE RULE of cp_ccl_instance_labels:
 *   - a component is a 4-connected set of pixels with equal labels in 1..objects (a label above `objects` is background, as in
 *     cp_ccl_filter_labels);
 *   - a component is eligible when it has at least min_size pixels;
 *   - the eligible components of an object are ordered by size descending, then by root ascending, the root being the raster index of the
 *     component's first pixel;
 *   - instance r (0-based) of object o (1-based) gets the slot id (o-1)*R + r + 1;
 *   - a pixel of an ineligible component, or of an eligible one ranked R or later, gets slot 0.
 * Two deliberate differences from the reference's histogram rule (:64-76), which cp_ccl_filter_labels restates with its quirks: there is no
 * "bin 0", so an object larger than the rest of the image is kept (the reference drops it); and an object whose components are all below
 * min_size keeps nothing (the reference keeps the first one in raster order).
 *   labels_in  uint8 [n,h,w]                    slots_out  uint8 [n,h,w]  the slot map
 *   inst_out   int32 [n][objects][R][2]         (size, image-local root y*w + x) of every slot, (0, -1) for an empty one; every word is written
 *   ws         cp_ccl_instance_workspace_bytes(n, h, w, objects, R) bytes; needs no initialisation
 * 1 <= R <= 16 and objects * R <= 254 (slot ids are bytes); anything else is refused before any launch, and
 * cp_ccl_instance_workspace_bytes returns 0 for it.  Integer atomics only: two calls with the same input give the same bytes.
 *
 * cp_ls_vote_slots_f32 is cp_ls_vote_w_f32 with given labels, except that the table has `slots` rows (1..254) whatever the record's class
 * count, slot_map is required (values 0..slots, 0 = no vote), and no logits are read: there is no seg_off.  A value above `slots` is the
 * caller's error, exactly as a label above `objects` is for cp_ls_vote_w_f32: the production record's kernel reads it as 0, on every other
 * layout (the generic kernel, which cp_ls_vote_w_f32 shares and which uses the byte as its table row) the result is undefined.
 * cp_ccl_instance_labels never writes such a value.  sums_ws: fp64 [n][slots][kp][5] of
 * cp_ls_vote_workspace_bytes(n, slots, kp) bytes (zeroed by the call); keypoints: fp32 [n][slots][kp][2] in (y,x) pixels, (0, 0) for a slot
 * without pixels.  The production record (ld 36, dir_off 9, conf_off 27, softplus weights) has a kernel of its own for any slot count; every
 * other layout takes the generic kernel.  The LDS table of slots * kp * 5 doubles lies beside the staging buffer of 1024 * ld bytes; the
 * largest combination (254 slots beside ld = 64) takes 156 976 of the 160 KB a workgroup may have.
 * Added in ABI 302 without changing any earlier entry point. */
int cp_ccl_instance_labels(const uint8_t* labels_in, int batch, int h, int w, int objects, int max_instances, int min_size, void* ws,
                           uint8_t* slots_out, int32_t* inst_out, void* stream);
size_t cp_ccl_instance_workspace_bytes(int batch, int h, int w, int objects, int max_instances);
int cp_ls_vote_slots_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w, int slots,
                         int kp, int sigmoid_weights, double* sums_ws, float* keypoints, void* stream);

/* ---- touching instances of one object, split by their centre votes (csrc/vote_split.hip, csrc/vote_split_math.h) ---------------------------
 * cp_ccl_instance_labels cannot separate two instances of one object that touch: they are one component.  Keypoint 0 of every object is its
 * box centre, so every pixel carries a direction to its OWN instance's centre; cp_vote_split_labels lets the pixels vote for that centre on a
 * coarse grid (a Hough step), takes up to R peaks per object and gives every pixel to the peak its direction points at.  The slot map and the
 * slot ids are cp_ccl_instance_labels'; cp_ls_vote_slots_f32 consumes them unchanged.
 *
 * THE RULE of cp_vote_split_labels.  All fp32 arithmetic is one rounding per operation, without contraction; division is correctly rounded;
 * every integer result is independent of the order of summation.
 *   inputs   labels uint8 [n,h,w] (a label above `objects` is background); field fp32 [n,h,w,ld]; the direction d = (dy, dx) of a pixel are
 *            the floats dir_off + 2*kp_index and the next one of its record (kp_index 0 = the centre); R = max_instances in 1..16 with
 *            objects * R <= 254; cell in {2, 4, 8}; vote_stride 1..4; min_votes >= 1; rel_percent 0..100; nms_radius 1..4 cells; gate > 0 in
 *            pixels (fp32); min_size >= 1.
 *   1. accumulate   acc is int32 [n][objects][gh][gw], gh = ceil(h/cell), gw = ceil(w/cell), zeroed by the call.  A pixel (y, x) votes when
 *            y % vote_stride == 0, x % vote_stride == 0, its label l is in 1..objects, both components of d are finite and d != (0, 0).  The
 *            major axis is y when |dy| >= |dx|, else x; m = d_minor / d_major; s = +1 when d_major > 0, else -1; a0 = major + 0.5,
 *            b0 = minor + 0.5.  For k = 0, 1, 2, ...: t = s * float(cell*k), a = a0 + t, b = b0 + t*m (the product rounded, then the sum).
 *            The ray stops at the first k with (a, b) outside [0, extent_major) x [0, extent_minor); before that
 *            acc[l-1][floor(a/cell), floor(b/cell)] += 1, the pair mapped back to (cy, cx).  Step 0 is the pixel's own cell.
 *   2. peaks, per (image, object)   the key of a cell is (votes << 32) | (0xFFFFFFFF - (cy*gw + cx)).  A cell is a candidate when
 *            votes >= min_votes and its key is the largest in its (2*nms_radius+1)^2 window clipped to the grid.  The R candidates with the
 *            largest keys are ranked in that order, rank r = the position; every one with votes*100 < rel_percent*top_votes (top_votes: rank
 *            0's) is dropped.  The peak position is taken in fp64 over the clipped 3 x 3 cells around the peak:
 *            py = (double)sum(v*(2*cy_i+1)) / (double)sum(v) * (0.5*cell), rounded to fp32, the sums being integers; px likewise.
 *   3. assign   a pixel of label l (EVERY pixel, whatever vote_stride) compares the peaks of object l in rank order, in fp32 and in this order:
 *            e = peak - pixel centre; e2 = ey*ey + ex*ex; n2 = dy*dy + dx*dx; dot = ey*dy + ex*dx; cr = ey*dx - ex*dy;
 *            dist2 = cr*cr / n2 when n2 is finite, n2 > 0 and dot > 0, otherwise dist2 = e2.  The pixel takes the peak with the smallest
 *            dist2 among those with dist2 <= gate*gate, the lower rank on a tie, and the slot id (l-1)*R + r + 1; with none it takes slot 0.
 *   4. size gate   a slot with fewer than min_size assigned pixels is emptied: its pixels become 0.  Slots are not renumbered.
 *   outputs  slots_out uint8 [n,h,w]; inst_out int32 [n][objects][R][4] = (pixels, votes, peak cy, peak cx): (0, 0, -1, -1) for a rank
 *            without a peak, (0, votes, cy, cx) for one emptied by step 4, every word written; peaks_out fp32 [n][objects][R][2] = (y, x),
 *            (0, 0) where there is no peak.
 *   ws       cp_vote_split_workspace_bytes(n, h, w, objects, R, cell) bytes, 16-byte aligned; needs no initialisation.  After the call it holds
 *            acc and, as uint64 [n][objects][gh][gw], every candidate's key (0 for a cell that is none) at the byte offsets
 *            cp_vote_split_workspace_layout writes to offsets[0] and offsets[1]; offsets[2] is where the slots' pixel counts before step 4
 *            lie, int32 [n][objects*R].  The layout function runs on the host and launches nothing.
 * Further limits: h, w <= 16384; one object's grid has at most 36864 cells (it lies in a workgroup's LDS: 480 x 640 needs cell >= 4);
 * n*h*w < 2^31.  Every size outside the limits is refused by name before any launch, and cp_vote_split_workspace_bytes returns 0 for it.
 * Integer atomics only, no floating-point atomics: two calls on equal inputs give equal bytes.  There is no host twin: the arithmetic's host
 * coverage is csrc/vote_split_selftest.cpp.  Added in ABI 302 without changing any earlier entry point. */
int cp_vote_split_labels(const uint8_t* labels, const float* field, int ld, int dir_off, int kp_index, int batch, int h, int w, int objects,
                         int max_instances, int cell, int vote_stride, int min_votes, int rel_percent, int nms_radius, float gate, int min_size,
                         void* ws, uint8_t* slots_out, int32_t* inst_out, float* peaks_out, void* stream);
size_t cp_vote_split_workspace_bytes(int batch, int h, int w, int objects, int max_instances, int cell);
int cp_vote_split_workspace_layout(int batch, int h, int w, int objects, int max_instances, int cell, size_t* offsets /*[3]*/);

/* ---- the robust LS voter per slot: reweighted passes reject stray pixels (csrc/ls_vote.hip, csrc/ls_robust_math.h) ---------------------------
 * A slot map hands a few pixels to the wrong slot (beside the contact of two touching instances, or where the segmentation is wrong); they
 * carry another instance's directions and the least-squares voter counts them in full.  cp_ls_vote_slots_robust_f32 votes as
 * cp_ls_vote_slots_f32 does (same arguments, same refusals, same kernels for pass 0) and then repeats the vote `passes` times with every
 * (pixel, keypoint) term multiplied by rho, Tukey's biweight of the perpendicular distance of the CURRENT estimate from the pixel's line:
 *     c = ((y + .5) / h, (x + .5) / h);  n = the pixel's unit direction;  p = the keypoint of the pass before / h (fp32);  e = p - c;
 *     t = (e_y n_x - e_x n_y) * (h / cutoff_px);  u = t * t;  rho = u < 1 ? (1 - u)^2 : 0          (fp32, in this order)
 * and the term is ls_add_terms' with w * rho in place of w.  A pixel whose direction is (0, 0) has no line: rho = 0 (the plain pass counts it
 * as w I, as before).  There is no "behind the ray" rule.
 *   workspace  cp_ls_vote_robust_workspace_bytes(n, slots, kp) bytes, 8-byte aligned, no initialisation needed: two blocks fp64
 *              [n][slots][kp][5].  After the call block 0 holds the plain sums (cp_ls_vote_slots_f32's sums_ws), block 1 the reweighted sums
 *              of the last pass (not written with passes = 0: that call launches exactly what cp_ls_vote_slots_f32 launches).
 *   keypoints  fp32 [n][slots][kp][2] in (y,x) pixels, 8-byte aligned: the last pass's values; (0, 0) for a slot without pixels.
 *   passes     0..8; 0 gives cp_ls_vote_slots_f32's keypoints (the same kernels on the same input).   cutoff_px  finite and > 0, in pixels.
 * The solve of a reweighted pass, per (image, slot, keypoint): the new value is taken when the reweighted 2 x 2 system passes the plain solve's
 * rank rule, its condition number is below 1e6, and its trace S00 + S11 is at least CP_LS_ROBUST_MIN_KEPT = 1/8 of the plain system's trace
 * (ny^2 + nx^2 = 1, so the trace of a system is the weight it holds); otherwise the keypoint keeps the value of the pass before.  No state is
 * kept: the next pass starts from the same estimate and decides the same.  trace(block 1) / trace(block 0) is the share of the plain weight
 * the last pass kept.  Every (slots, ld) cp_ls_vote_slots_f32 accepts is accepted: the estimates of a lane's current slot live in registers.
 * A slot value above `slots` is the caller's error as it is for cp_ls_vote_slots_f32.  Added in ABI 302 without changing any earlier entry
 * point. */
size_t cp_ls_vote_robust_workspace_bytes(int batch, int slots, int kp);
int cp_ls_vote_slots_robust_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w, int slots,
                                int kp, int sigmoid_weights, float cutoff_px, int passes, void* workspace, float* keypoints, void* stream);

/* ---- a covariance per slot and keypoint from the LS objective itself (csrc/ls_vote.hip, csrc/ls_cov_math.h) ---------------------------------
 * cp_ls_slot_covariance_f32 says how far each keypoint of each slot can be trusted, for keypoints HANDED IN (either slot voter's, or any
 * other): one more stream over the labelled pixels (the walk of a reweighted pass) and a finish per keypoint.  Nothing an earlier call summed
 * is read, no state is kept.  The arguments up to sigmoid_weights are cp_ls_vote_slots_f32's, with the same refusals.
 * THE RULE, per (image, slot, keypoint) with the estimate p = keypoint / h (fp32).  For every pixel of the slot whose direction is not (0, 0),
 * in fp32 and in this order:
 *     c = ((y + .5) / h, (x + .5) / h);  n = the pixel's unit direction;  e = p - c;  d = e_y n_x - e_x n_y;
 *     rho = Tukey's biweight of d * (h / cutoff_px) as cp_ls_vote_slots_robust_f32 forms it when cutoff_px > 0, otherwise 1;
 *     omega = w * rho;   the matrix terms (1 - ny^2) omega, (0 - ny nx) omega, (1 - nx^2) omega;   q = omega * (d * d)
 * summed in fp64 into sums_ws = (A00, A01, A11, Q, Wall), Wall the sum of w before reweighting.  A pixel with direction (0, 0) takes no part in
 * any of the five, with or without a cut-off (the plain vote counts it as w I).  The finish, in fp64:
 *     W = A00 + A11;   sigma2 = h^2 Q / W;   kept = W / Wall;   Sigma = sigma2 (A / W)^-1 = h^2 Q A^-1
 * Sigma is the covariance of ONE vote of average weight, in pixels^2: the scale of a hypothesis scatter, long along the rays of a keypoint far
 * from the slot's pixels.  It is not the standard error of the estimate.  A truncated Tukey residual underestimates sigma2; not corrected.
 *   cutoff_px  finite and >= 0, in pixels; 0 means no reweighting.
 *   keypoints  in, fp32 [n][slots][kp][2] in (y,x) pixels, 8-byte aligned; not written.
 *   sums_ws    cp_ls_vote_workspace_bytes(n, slots, kp) bytes, 8-byte aligned, no initialisation needed; holds the five sums afterwards.
 *   cov        out, fp32 [n][slots][kp][3] = (sxx, sxy, syy) in the (x,y) pixels cp_pnp_weighted_f64 reads: (Sigma[1][1], Sigma[0][1],
 *              Sigma[0][0]) of the (y,x) matrix.  Three NaNs (which the weighted PnP refuses: the pair is solved unweighted and says so) where
 *              A fails the rank rule or the condition bound 1e6 of the robust voter's solve, kept < CP_LS_ROBUST_MIN_KEPT = 1/8, the keypoint
 *              is not finite, or W is not > 0 (a slot without pixels).
 *   stat       out, fp32 [n][slots][kp][2] = (sigma2, kept); (0, 0) where W is not > 0 or the keypoint is not finite.
 * A slot value above `slots` is background.  Added in ABI 302 without changing any earlier entry point. */
int cp_ls_slot_covariance_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w, int slots,
                              int kp, int sigmoid_weights, float cutoff_px, const float* keypoints, double* sums_ws, float* cov, float* stat,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASAPOSE_HIP_H */
