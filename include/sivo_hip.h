/*
 * sivo_hip.h — C ABI of libsivo_hip.so: the MI355X (gfx950) implementation of
 * navganti/SIVO's per-frame perception hot path.
 *
 * The reference has no FFI layer: its seam is the C++ class API of three
 * shared libraries (reference CMakeLists.txt:74-123).  Every entry point below
 * names the reference interface it stands behind; the C++ classes with the
 * reference's own signatures (sivo_amd/api/) are thin callers of this ABI, and
 * INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions: plain pointers and sizes only; `int` status (0 = ok); no
 * exceptions cross the boundary; `*_dev` entry points take DEVICE pointers and
 * a hipStream_t passed as void* (NULL = the default stream) and never
 * synchronise; the others take HOST pointers and return when the result is
 * ready.  Handles are not re-entrant (reference BayesianSegNet::segmentImage
 * mutates a shared input blob too); distinct handles may be used from
 * distinct host threads (reference Frame.cc:126-129 runs two ORBextractors
 * concurrently).
 */
#ifndef SIVO_HIP_H
#define SIVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIVO_OK 0
#define SIVO_ERR_INVALID_ARGUMENT 1 /* the C++ classes rethrow this as std::invalid_argument
                                       (reference bayesian_segnet.cpp:65-70,80-89) */
#define SIVO_ERR_RUNTIME 2          /* HIP error / no device */
#define SIVO_ERR_UNSUPPORTED 3      /* layer type or shape outside the two reference nets' vocabulary */
#define SIVO_ERR_IMAGE_TOO_SMALL 4  /* reference resizeImage returns an empty Mat (bayesian_segnet.cpp:142-162) */
#define SIVO_ERR_CAPACITY 5         /* caller buffer too small */

/* Thread-local text of the last failure on this thread. */
const char *sivo_last_error(void);
int sivo_version(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int sivo_device_count(void);

/* ===========================================================================
 * Bayesian SegNet — stands behind SIVO::BayesianSegNet
 * (reference include/bayesian_segnet/bayesian_segnet.hpp:108-170,
 *  src/bayesian_segnet/bayesian_segnet.cpp:46-78, 299-318).
 * ======================================================================== */
typedef struct sivo_segnet *sivo_segnet_t;

/* BayesianSegNet::BayesianSegNet (bayesian_segnet.cpp:46-78): parse the Caffe
 * prototxt text, take T,C,H,W from the input blob, upload the parameters.
 * `weights` is the flat fp32 parameter array in prototxt layer order
 * (Convolution: W[Cout][Cin][k][k] then bias[Cout]; BN: scale[C] then
 * shift[C]).  t_override > 0 replaces the prototxt batch size (the standard
 * prototxt ships with it blank).  Errors: empty text / C != 3 / T <= 1 ->
 * SIVO_ERR_INVALID_ARGUMENT, as the reference constructor throws. */
int sivo_segnet_create(const char *prototxt_text, size_t prototxt_len, int t_override,
                       const float *weights, size_t n_weights, int device, sivo_segnet_t *out);
/* How a handle runs, chosen by the caller at construction (the fields BayesianSegNetParams gains in sivo_amd/api/bayesian_segnet:
 * the reference's params struct, include/bayesian_segnet/bayesian_segnet.hpp:23-40, holds the two file names only).  The library reads
 * NO environment variable: every sivo_segnet_create* has an `_opts` twin taking this struct (NULL = the defaults below, which is also
 * what the plain functions use).  Zero-initialise, set struct_size = sizeof(SivoSegnetOptions), fill what differs from the default. */
typedef struct SivoSegnetOptions {
    uint32_t struct_size;        /* sizeof(SivoSegnetOptions) of the caller's header: fields beyond it take their defaults */
    int32_t lanes;               /* sample groups of the per-sample part on separate HIP streams: 1..4; 0 = default (2) */
    int32_t gemm;                /* arithmetic of the matrix-core layers: 0 = default f16x3 (fp32 operands as fp16 hi + lo, 3 products);
                                    1 = bf16x6; 2 = fp32 MFMA.  1 and 2 also turn the direct f16x3 kernels and the f16x3 classifier off */
    int32_t no_direct_f16x3;     /* != 0: the direct f16x3 3x3 / 7x7 kernels and the f16x3 classifier off (the fp32 fused kernels instead) */
    int32_t no_packed_activations; /* != 0: fp32 blobs between the direct f16x3 layers instead of packed fp16 hi | lo pieces */
    int32_t conv7_fp32;          /* != 0: SegNet-Basic's 7x7 layers on the fp32 matrix cores */
    int32_t wino4_workspace_mb;  /* workspace budget of the three-kernel F(4x4) path in MiB; 0 = default (16384) */
    int32_t debug_sync;          /* != 0: a device synchronisation behind every op of every lane (debugging) */
} SivoSegnetOptions;
int sivo_segnet_create_opts(const char *prototxt_text, size_t prototxt_len, int t_override, const float *weights, size_t n_weights,
                            int device, const SivoSegnetOptions *opts, sivo_segnet_t *out);
/* Caffe's Net::CopyTrainedLayersFrom (called at bayesian_segnet.cpp:61): read a
 * trained `.caffemodel` (binary protobuf NetParameter; both the `layer` and the
 * legacy `layers` encodings), match its layers to the prototxt BY NAME and write
 * the flat parameter array sivo_segnet_create takes.  Host-only (no GPU needed).
 * *n_weights receives the count; `out` may be NULL to query it; capacity <
 * count -> SIVO_ERR_CAPACITY.  A layer missing from the file or with blobs of the
 * wrong size -> SIVO_ERR_INVALID_ARGUMENT (Caffe CHECK-fails there). */
int sivo_caffemodel_weights(const char *prototxt_text, size_t prototxt_len, const void *model_bytes,
                            size_t model_len, float *out, size_t capacity, size_t *n_weights);
/* Same from files: model_file = prototxt, weights_file = the reference's
 * `.caffemodel` or a .sivow container (sivo_amd/weights.py).  Empty paths -> SIVO_ERR_INVALID_ARGUMENT
 * (bayesian_segnet.cpp:80-89, pinned by tests/test_bayesian_segnet.cpp:138-150). */
int sivo_segnet_create_from_files(const char *model_file, const char *weights_file, int t_override,
                                  int device, sivo_segnet_t *out);
int sivo_segnet_create_from_files_opts(const char *model_file, const char *weights_file, int t_override, int device,
                                       const SivoSegnetOptions *opts, sivo_segnet_t *out);
/* The same network with the T Monte-Carlo samples of a frame spread over several GPUs INSIDE the handle (the reference
 * constructs one BayesianSegNet, src/orbslam/System.cc:94-95, so a multi-GPU drop-in has to live behind that object).
 * One process; every device holds the full weights and takes a contiguous share of the samples (dropout keyed by the
 * global sample index); per frame: local softmax sums -> RCCL reduce-scatter over pixel ranges (fp32) -> every device
 * finalizes its 1/ndev of the pixels in f64 -> RCCL all-gather of the class / confidence / entropy chunks -> device
 * device_ids[0] hands the maps to the caller.  H*W must be a multiple of ndev, T >= ndev, devices distinct.
 * Only sivo_segnet_segment, _shape, _num_devices and _destroy take such a handle.  librccl.so is opened on first use. */
int sivo_segnet_create_multi(const char *prototxt_text, size_t prototxt_len, int t_override, const float *weights,
                             size_t n_weights, const int *device_ids, int ndev, sivo_segnet_t *out);
/* The same from the two files of BayesianSegNetParams (bayesian_segnet.hpp:23-40), like sivo_segnet_create_from_files. */
int sivo_segnet_create_multi_from_files(const char *model_file, const char *weights_file, int t_override,
                                        const int *device_ids, int ndev, sivo_segnet_t *out);
int sivo_segnet_create_multi_opts(const char *prototxt_text, size_t prototxt_len, int t_override, const float *weights, size_t n_weights,
                                  const int *device_ids, int ndev, const SivoSegnetOptions *opts, sivo_segnet_t *out);
int sivo_segnet_create_multi_from_files_opts(const char *model_file, const char *weights_file, int t_override, const int *device_ids,
                                             int ndev, const SivoSegnetOptions *opts, sivo_segnet_t *out);
int sivo_segnet_num_devices(sivo_segnet_t h, int *ndev);
int sivo_segnet_destroy(sivo_segnet_t h);
/* getInputGeometry (bayesian_segnet.hpp) and the blob shapes: T, C(=3), H, W, classes. */
int sivo_segnet_shape(sivo_segnet_t h, int32_t *T, int32_t *C, int32_t *H, int32_t *W, int32_t *classes);
/* Number of fp32 parameters the prototxt implies (size of `weights`). */
int sivo_segnet_num_params(const char *prototxt_text, size_t prototxt_len, size_t *n_params);

/* network->Forward() (bayesian_segnet.cpp:310) for `n_samples` Monte-Carlo
 * samples with global indices sample0 .. sample0+n_samples-1 (the T samples
 * of one frame are sharded over ranks this way; n_samples <= T).
 *   d_bgr       device, H*W*3 u8, BGR interleaved, already cropped to H x W
 *               (preprocessImage, :164-178: no scaling, no mean)
 *   d_prob_sum  device, classes*H*W fp32: sum over the n_samples of the
 *               per-pixel softmax (the tensor the all-reduce carries), accumulated
 *               in f64 and rounded once to fp32; the mean of extractMeanConfidence
 *               (:278-297) is this / T_total up to that rounding (6e-8 relative; the
 *               single-device entry points sivo_segnet_segment[_dev] keep f64 throughout)
 *   d_logits    device or NULL, n_samples*classes*H*W fp32 pre-softmax scores
 *   d_prob      device or NULL, n_samples*classes*H*W fp32 softmax ("prob" blob)
 * Dropout masks: Philox4x32-10 keyed on (seed; site, global sample, element). */
int sivo_segnet_forward_dev(sivo_segnet_t h, const uint8_t *d_bgr, int n_samples, int sample0,
                            uint64_t seed, float *d_prob_sum, float *d_logits, float *d_prob,
                            void *stream);

/* computeClasses / computeMaxConfidence / computeClassificationEntropy
 * (bayesian_segnet.cpp:180-203, 262-276) from the probability sum:
 * mean = sum / t_total in f64; argmax (first maximum wins), max, and
 * sum_c (p == 0 ? 0 : -p*log2 p). */
int sivo_mc_finalize_dev(const float *d_prob_sum, int classes, int64_t hw, int t_total,
                         uint8_t *d_classes, double *d_confidence, double *d_entropy, void *stream);

/* ---- The sample-invariant prefix split into row bands over the ranks that share a frame's samples (the reference has one
 * device and no such split: bayesian_segnet.cpp:174-177 copies the image T times and Caffe computes the encoder T times).
 * With the T samples sharded over `world` ranks (sivo_segnet_forward_dev with n_samples / sample0) every rank would recompute the
 * whole prefix (everything in front of the first test-time Dropout: conv1_1 .. pool3 in SegNet-Standard).  Instead rank r computes
 * the rows rows[r] .. rows[r + 1] of the prefix output from a band of the image (input_rows[2 r] .. input_rows[2 r + 1]: its rows
 * plus the receptive-field halo) and packs what the per-sample part reads of the prefix — the pooled values in front of the dropout
 * and the pooling masks — into a slot of *slot_bytes; ONE all-gather of the slots (rank order) replaces the recomputation:
 *     sivo_segnet_prefix_bands(h, world, &slot_bytes, rows, input_rows);            // once
 *     sivo_segnet_prefix_band_dev(h, d_bgr, rank, world, d_my_slot, stream);        // per frame: my band
 *     ... all-gather: d_slots = world slots in rank order (RCCL / torch.distributed) ...
 *     sivo_segnet_forward_banded_dev(h, d_slots, world, n_samples, sample0, seed, d_prob_sum, NULL, stream);
 * The results are bit-identical to sivo_segnet_forward_dev on the whole image (tests/test_gpu_prefix_bands.py): a band's valid
 * rows do not depend on the band.  The last H_out % world ranks take one row more (rank 0 the lighter share).
 * fp16 range guard across ranks: a band that leaves the fp16 range raises the flag of ITS rank's handle only
 * (sivo_segnet_take_overflow == 1 there), but every rank has consumed its rows.  The caller must OR-reduce the answers of
 * sivo_segnet_take_overflow over the ranks once per frame; when any rank says 1, EVERY rank reissues the frame (band, all-gather,
 * forward) — handles that said 0 have not backed off and keep their scales, which is the one situation in which the ranks'
 * arithmetic differs (each within tolerance, no longer bit-identical to the whole-image forward) until those handles are rebuilt;
 * bench.py --gpus N reduces the flag and refuses to report a rate containing such a frame.  The in-handle multi-device form
 * (sivo_segnet_create_multi) does all of this itself: every device backs off once per event and the frame is recomputed. */
int sivo_segnet_prefix_bands(sivo_segnet_t h, int world, size_t *slot_bytes, int32_t *rows, int32_t *input_rows);
int sivo_segnet_prefix_band_dev(sivo_segnet_t h, const uint8_t *d_bgr, int rank, int world, void *d_slot, void *stream);
int sivo_segnet_forward_banded_dev(sivo_segnet_t h, const void *d_slots, int world, int n_samples, int sample0, uint64_t seed,
                                   float *d_prob_sum, float *d_logits, void *stream);
/* Softmax over the class axis of (n, classes, hw) logits and sum over n
 * (Softmax layer + the sum half of extractMeanConfidence).  accumulate != 0
 * adds to d_prob_sum instead of overwriting it. */
int sivo_mc_reduce_dev(const float *d_logits, int n, int classes, int64_t hw, float *d_prob_sum,
                       float *d_prob, int accumulate, void *stream);

/* computeVariance (bayesian_segnet.cpp:205-260; private and unused in the
 * reference): sample variance over T of the winning class's probability. */
int sivo_mc_variance_dev(const float *d_prob, int T, int classes, int64_t hw, const uint8_t *d_classes,
                         double *d_variance, void *stream);

/* BayesianSegNet::segmentImage (bayesian_segnet.cpp:299-318), host buffers:
 * centre-crop (resizeImage :142-162), upload, T samples, finalize, download.
 * classes: H*W u8, confidence / entropy: H*W f64 (row-major, like MatXu/MatXd). */
int sivo_segnet_segment(sivo_segnet_t h, const uint8_t *bgr_hwc, int rows, int cols, uint64_t seed,
                        uint8_t *classes, double *confidence, double *entropy);

/* segmentImage with the frame already in HBM and the maps left there (no synchronisation): all T samples, then the
 * mean over the T float probabilities in f64 exactly as extractMeanConfidence (bayesian_segnet.cpp:278-297) — the
 * probability sum never goes through fp32 memory — and classes / confidence / entropy.  d_bgr: H*W*3 u8. */
int sivo_segnet_segment_dev(sivo_segnet_t h, const uint8_t *d_bgr, uint64_t seed, uint8_t *d_classes,
                            double *d_confidence, double *d_entropy, void *stream);

/* The same, and additionally the logits (T, classes, H, W fp32, the "conv1_1_D" blob of the reference's net) the maps
 * were computed from.  When the net ends in a 3x3 classifier convolution, segment / segment_dev / forward_dev (without
 * d_logits / d_prob) run that convolution, the Softmax layer and the reduction over the samples as ONE kernel
 * (conv_cls_mc.hip) and the logits never reach memory; this entry point makes that kernel also store them, so a test can
 * check (a) the logits against the reference net and (b) the maps against sivo_mc_segment_dev of exactly these logits.
 * Test/diagnostic entry point (adds T x 21.6 MB of stores per frame). */
int sivo_segnet_segment_logits_dev(sivo_segnet_t h, const uint8_t *d_bgr, uint64_t seed, uint8_t *d_classes,
                                   double *d_confidence, double *d_entropy, float *d_logits, void *stream);

/* The post-processing of segmentImage on given network outputs (bayesian_segnet.cpp:299-318 after Forward():
 * extractMeanConfidence :278-297, computeClasses :180-190, computeMaxConfidence :192-203,
 * computeClassificationEntropy :262-276): per pixel the Softmax of each of the T samples' logits (fp32), the mean of the T
 * float probabilities in f64, its argmax (first maximum wins), maximum and entropy in bits.  d_logits: (T, classes, hw). */
int sivo_mc_segment_dev(const float *d_logits, int T, int classes, int64_t hw, uint8_t *d_classes,
                        double *d_confidence, double *d_entropy, void *stream);

/* Copy a named blob of the last forward to the host (fp32; pooling masks are
 * returned as the flat input-plane index Caffe stores, as fp32).  shape =
 * {N, C, H, W}.  Test/diagnostic entry point.  Blobs that only exist on chip (fused away) are refused; the logits blob
 * (input of the Softmax layer) is written only by passes that ask for logits or per-sample probabilities
 * (sivo_segnet_forward_dev with d_logits / d_prob): segment / segment_dev / forward_dev without them run the classifier
 * fused with the Monte-Carlo post-processing and leave that blob as the last such pass wrote it. */
int sivo_segnet_blob(sivo_segnet_t h, const char *name, float *host_out, size_t capacity, int32_t shape[4]);

/* Algorithmic FLOPs of one forward (2*k*k*Cin*Cout*H*W per conv): shared =
 * the sample-invariant prefix, per_sample = the rest. */
int sivo_segnet_flops(sivo_segnet_t h, double *shared, double *per_sample);

/* Per-layer timing with HIP events recorded on the launch stream around every
 * kernel of the forward (enable: 0 off, 1 on, 2 on + reset).  Timings are
 * harvested lazily (at the next forward or at profile_read). */
typedef struct {
    char layer[64];          /* prototxt layer name of the (fused) op */
    char kernel[96];         /* kernel symbol as rocprofv3 --kernel-trace prints it (sivo:: prefix omitted) */
    int32_t samples;         /* batch of the last launch: 1 for the shared prefix, n_samples otherwise */
    int32_t launches;
    double flops_per_sample; /* algorithmic FLOPs of one sample (convolutions; 0 otherwise) */
    double bytes_per_sample; /* algorithmic HBM bytes of one sample */
    double ms_total;         /* sum of the event-timed durations of all harvested launches */
    int32_t kernel_launches; /* kernel launches behind `launches` forward passes (an F(4x4,3x3) layer runs its three
                              * kernels once per sample group and reports them as three rows) */
    int32_t pad_;
} SivoOpProfile;
/* enable: 0 off (does not wait for the events of the last profiled forward: they are harvested by the next sivo_segnet_profile_read or
 * before profiling is switched on again); 1 on; 2 on + reset the accumulators; 3 like 2 but only the MFMA kernels are bracketed (convolution
 * kernels and the F(4x4,3x3) GEMM): a handful of events per forward, for timing inside a throughput run; 4 like 3
 * without the reset (to profile a subset of the frames of a run); 5 / 6 like 3 / 4, but the profiled forward KEEPS its sample groups
 * on their streams (modes 1 - 4 run it in one lane, one launch per layer, so that a launch has the GPU to itself): events per lane,
 * ms_total is the sum over the lanes — the kernel's time while it shares the chip with the other lane. */
int sivo_segnet_profile(sivo_segnet_t h, int enable);
int sivo_segnet_profile_read(sivo_segnet_t h, SivoOpProfile *out, int capacity, int *n_out);

/* The arithmetic the matrix-core layers of the handle run: *mode = 2 f16x3 (fp32 operands as fp16 hi + lo planes, three
 * products: the default), 1 bf16x6 (three bf16 planes, six products: SIVO_GEMM=x6, and a handle whose fourth frame raised
 * the fp16 overflow flag), 0 fp32 MFMA (SIVO_GEMM=f32) or no such layer.  *overflow_frames = frames in which a value times
 * its layer's scale left the fp16 range since the handle was created.  Such a frame is wrong.  sivo_segnet_segment recomputes
 * it (without f16x3) before it returns; the asynchronous *_dev entry points cannot: once the caller has synchronised with the
 * frame it asks sivo_segnet_take_overflow, and if that says 1 it issues the same call again — that call runs without f16x3.
 * After every such frame the handle lowers its f16x3 scales by 2^2 (two more bits of headroom) and stays on f16x3; the
 * fourth switches it to bf16x6 / fp32 kernels for good.
 * per_layer (optional): one row per f16x3-capable layer with the calibration's largest |V| (three synthetic frames x MC
 * samples 0..11) and the powers of two in use for V and U; *n_layers = rows available. */
typedef struct SivoH3Layer {
    char layer[48];
    float vmax, vscale, uscale;
} SivoH3Layer;
int sivo_segnet_gemm_status(sivo_segnet_t h, int *mode, int *overflow_frames, SivoH3Layer *per_layer, int capacity, int *n_layers);
/* The load-time accuracy guard of the matrix-core layers.  At construction every 3x3 layer the plan runs on Winograd
 * F(4x4,3x3) or on the fp16 hi + lo split is evaluated on two built-in calibration frames x MC samples 0, 1 beside the direct fp32
 * kernel, on the same input: rel_err = max |layer - direct fp32| / max |direct fp32| (rel_rms the same in rms).  *predicted =
 * 0.5 sqrt(sum rel_err^2) estimates the error of the logits relative to their scale; *budget = 1e-3 / 30 (the tolerance at the
 * logit range of the reference configuration).  While the prediction was above the budget (a third of it, once a plan has needed
 * correction) the largest contributors were moved one level down and the handle planned again (*builds plans in all): level 0 as planned, 1 off F(4x4) (direct f16x3), 2 off
 * f16x3 as well (F(2x2) / direct fp32), 3 direct fp32 only.  Rows describe the FINAL plan (kernel = what the layer runs now);
 * first_rel_err = what the layer measured in the first plan.  *logit_max = largest |logit| of the guard's frames.
 * *guard_ms = wall time the guard added to construction; nothing runs per frame.  *predicted > *budget with *builds == 5: the guard
 * ran out of plans with the last one still over its budget (also written to stderr at construction).  No rows: nothing to guard, or the guard
 * was skipped (diagnostic build SIVO_GUARD=0; scales forced out of the fp16 range). */
typedef struct SivoGuardLayer {
    char layer[48];
    char kernel[24];
    float rel_err, rel_rms, ref_max, first_rel_err;
    int32_t level;
} SivoGuardLayer;
int sivo_segnet_guard_report(sivo_segnet_t h, SivoGuardLayer *rows, int capacity, int *n_rows, float *budget, float *predicted,
                             float *logit_max, double *guard_ms, int *builds);
/* *overflowed = 1 when a frame issued through an asynchronous entry point of this handle since the last call left the fp16
 * range: the handle has backed off as described above (once per event, however many frames in flight raised the flag) and its
 * NEXT forward runs without f16x3.  The answer is sticky: a later forward or status query that finds the flag first reacts
 * to it but leaves the report to this call, so with k frames in flight the caller that asks about frame i after frame i+1 was
 * issued still gets its 1.  The flag does not say WHICH frame: on 1, wait for every frame in flight, call this once more
 * (whatever they raised meanwhile belongs to the same event) and issue ALL of them again.
 * Reads one word of pinned host memory: free to call once per frame, after the frame's results were synchronised with. */
int sivo_segnet_take_overflow(sivo_segnet_t h, int *overflowed);

/* ===========================================================================
 * ORB extractor — stands behind SIVO::ORBextractor
 * (reference include/orbslam/ORBextractor.h:46-123, src/orbslam/ORBextractor.cc).
 * ======================================================================== */
typedef struct {  /* == cv::KeyPoint (28 bytes) */
    float x, y, size, angle, response;
    int32_t octave, class_id;
} SivoKeyPoint;

typedef struct sivo_orb *sivo_orb_t;

/* ORBextractor::ORBextractor (ORBextractor.cc:412-475). */
int sivo_orb_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast,
                    int device, sivo_orb_t *out);
int sivo_orb_destroy(sivo_orb_t h);
/* The GaussianBlur(7x7, sigma 2) in front of the descriptors (ORBextractor.cc:1060-1062) is OpenCV's, and its 8-bit taps differ
 * between the OpenCV versions README.md:57 admits ("> 3.2"): variant 0 (default) 18 34 49 55 49 34 18 — OpenCV 3.2 - 3.4.12 and
 * 4.0 - 4.5.0; variant 1 18 34 48 56 48 34 18 — OpenCV >= 3.4.13 / >= 4.5.1 (error-diffused taps, sum 256).  Pick the one the
 * reference build you compare against was linked with; descriptors are bit-exact per variant (INTEGRATION.md "OpenCV contract"). */
int sivo_orb_set_gaussian(sivo_orb_t h, int variant);
/* How an extraction is issued (round 6).  mode bits, each "this group of kernels in ONE launch": 0 ComputePyramid (ORBextractor.cc:1085-1122: a
 * workgroup recomputes the footprint of its tile on the levels above it in LDS, instead of one copy + nlevels - 1 dependent resizes), 1 FAST +
 * the scan of the cell counts + the ordered emission (ORBextractor.cc:775-819: a cell waits for the cells before it, instead of three
 * launches), 2 GaussianBlur + the reflect-101 borders, 3 IC_Angle + computeOrbDescriptor (one wave per keypoint).  Default 15: four launches
 * and NO copy per image (the kernels read the kept keys from, and write candidates and [angle | descriptor] records to, pinned host memory);
 * 0 = the fifteen launches of rounds 1 - 5.  Inside a frame whose network keeps every CU busy 14 is 0.6 % faster than 15 (the level-by-level
 * resize kernels need no LDS); results are bit-identical in every mode (tests/test_gpu_orb.py).
 * Bit 4 (value 16): the quadtree on the device.  After the FAST group (either form) one kernel distributes the candidates of every level,
 * one workgroup per level, reading candidates and offsets where FAST wrote them; the blur group and the angle / descriptor group follow, the
 * latter over fixed per-level slot ranges of max(features_per_level + 3, 4 * n_ini) keys whose waves past a level's count exit.  The host
 * waits ONCE, at the end, and reads the per-level counts, the kept words and the records; keys and descriptors are bit-identical to modes
 * 0 - 15 (tests/test_gpu_orb_quadtree.py).  An extractor whose nfeatures gives a level more than 2048 cells is refused
 * (SIVO_ERR_INVALID_ARGUMENT, the mode unchanged); a status word of the kernel -> SIVO_ERR_RUNTIME after both streams are drained.  The
 * default stays 15.  The call takes the handle's lock: it waits for a running extraction. */
int sivo_orb_set_launch_mode(sivo_orb_t h, int mode);
/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares + mnFeaturesPerLevel; arrays of nlevels. */
int sivo_orb_tables(sivo_orb_t h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                    int32_t *features_per_level);
/* ORBextractor::operator() (ORBextractor.cc:1019-1083): 8UC1 host image in,
 * keypoints (level 0 .. n-1 concatenated, pt scaled by the level factor) and
 * 32-byte descriptors out.  *n_out > capacity -> SIVO_ERR_CAPACITY. */
int sivo_orb_extract(sivo_orb_t h, const uint8_t *gray, int rows, int cols, int step,
                     SivoKeyPoint *keypoints, uint8_t *descriptors, int capacity, int *n_out);
/* Same with the image already resident in HBM (outputs still host). */
int sivo_orb_extract_dev(sivo_orb_t h, const uint8_t *d_gray, int rows, int cols, int step,
                         SivoKeyPoint *keypoints, uint8_t *descriptors, int capacity, int *n_out,
                         void *stream);
/* Both images of a stereo frame at once: Frame::Frame starts two ExtractORB threads and joins them (Frame.cc:126-131).  The right
 * extractor runs on a thread of the library's while the left one runs on the caller's; results as two sivo_orb_extract_dev calls. */
int sivo_orb_extract_pair_dev(sivo_orb_t left, sivo_orb_t right, const uint8_t *d_left, const uint8_t *d_right, int rows, int cols,
                              int step_left, int step_right, SivoKeyPoint *kp_left, uint8_t *desc_left, int capacity_left, int *n_left,
                              SivoKeyPoint *kp_right, uint8_t *desc_right, int capacity_right, int *n_right, void *stream);
/* Profiling of the extractor's kernels: enable != 0 brackets the kernel groups of every following extraction with HIP
 * events on the streams they run on and clears the accumulators.  sivo_orb_profile_read: mean ms per extraction of
 * ms5 = {pyramid (copy + resizes), blur + border, FAST cells + scan + compact, IC-angle, rBRIEF descriptors}, the number
 * of extractions measured and the mean number of keypoints. */
int sivo_orb_profile(sivo_orb_t h, int enable);
int sivo_orb_profile_read(sivo_orb_t h, double ms5[5], int *calls, double *mean_keys);

/* mvImagePyramid[level] (ORBextractor.h:83) of the last extraction: the level
 * image WITH its 19-pixel reflect-101 border, (rows+38) x (cols+38), tightly
 * packed; rows/cols report the interior size. */
int sivo_orb_level(sivo_orb_t h, int level, uint8_t *host_out, size_t capacity, int32_t *rows, int32_t *cols);
/* FAST candidates of one level of the last extraction (vToDistributeKeys,
 * ORBextractor.cc:765-819; coordinates relative to the 16-px border), in the
 * reference's emission order.  Test/diagnostic entry point. */
int sivo_orb_candidates(sivo_orb_t h, int level, SivoKeyPoint *out, int capacity, int *n_out);
/* DistributeOctTree (ORBextractor.cc:544-750), host only (sequential list surgery). */
int sivo_orb_distribute(const SivoKeyPoint *keys, int n, int min_x, int max_x, int min_y, int max_y,
                        int n_features, SivoKeyPoint *out, int capacity, int *n_out);
/* DistributeOctTree of n_sets candidate sets in one launch, one workgroup each; results equal sivo_orb_distribute on each set byte for byte.
 * Arrays are host arrays; set s is keys[set_off[s] .. set_off[s + 1]) in the region [min_x[s], max_x[s]) x [min_y[s], max_y[s]), its kept keys
 * are out[out_off[s] .. out_off[s + 1]).  A key must be what FAST produces (and what the kernel's packed word x:12 | y:12 | response:8
 * holds): integer-valued x in [0, max_x - min_x) and y in [0, max_y - min_y), both extents <= 4096, integer-valued response in [0, 256); the
 * other fields of a kept key are copied from its input key.  Refused with SIVO_ERR_INVALID_ARGUMENT and a message before any device is
 * touched: any other key, an empty region, round(W / H) < 1, n_features < 1, offsets that do not start at 0 or that decrease, NULL with a
 * non-zero count.  SIVO_ERR_CAPACITY: a set whose cell bound max(n_features + 3, 4 * n_ini) exceeds the kernel's table of 2048 cells
 * (before any device is touched), or more kept keys than out_capacity (out_off is still written).  Zero sets, or only empty sets, launch
 * nothing.  (How the rounds of the reference's loop become data-parallel steps: sivo_amd/csrc/orb_quadtree_math.hpp) */
int sivo_orb_distribute_batch_dev(int n_sets, const int64_t *set_off /* n_sets + 1 */, const SivoKeyPoint *keys,
                                  const int32_t *min_x, const int32_t *max_x, const int32_t *min_y, const int32_t *max_y,
                                  const int32_t *n_features, int64_t out_capacity, SivoKeyPoint *out,
                                  int64_t *out_off /* n_sets + 1 */, int device);

/* ===========================================================================
 * Hamming matching — stands behind SIVO::ORBmatcher
 * (reference include/orbslam/ORBmatcher.h:36-142, src/orbslam/ORBmatcher.cc).
 * Descriptors are rows of 32 bytes.
 * ======================================================================== */
/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:1582-1596), dense nA x nB. */
int sivo_hamming_matrix_dev(const uint8_t *d_a, int n_a, const uint8_t *d_b, int n_b, int32_t *d_out,
                            void *stream);
int sivo_hamming_matrix(const uint8_t *a, int n_a, const uint8_t *b, int n_b, int32_t *out);
/* Candidate-list argmin with best / second best (the inner loop of every
 * Search* routine, e.g. ORBmatcher.cc:78-104): for query i the candidates are
 * rows cand_idx[cand_off[i] .. cand_off[i+1]) of b, visited in order; ties keep
 * the earlier candidate; empty list -> idx -1, dist 256.  second_idx (may be
 * NULL) = the row that holds the second-best distance as the reference's scan
 * leaves it (its octave is what the ratio rule of ORBmatcher.cc:117-119 compares), -1 if none. */
int sivo_hamming_argmin2_dev(const uint8_t *d_a, int n_a, const uint8_t *d_b, const int32_t *d_cand_off,
                             const int32_t *d_cand_idx, int32_t *d_best_idx, int32_t *d_best_dist,
                             int32_t *d_second_dist, int32_t *d_second_idx, void *stream);
int sivo_hamming_argmin2(const uint8_t *a, int n_a, const uint8_t *b, int n_b, const int32_t *cand_off,
                         const int32_t *cand_idx, int32_t *best_idx, int32_t *best_dist,
                         int32_t *second_dist, int32_t *second_idx);
/* Brute-force argmin over ALL rows of b for every row of a (best, second). */
int sivo_hamming_bruteforce_dev(const uint8_t *d_a, int n_a, const uint8_t *d_b, int n_b,
                                int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_second_dist,
                                void *stream);

/* ---------------------------------------------------------------------------
 * Guided matching — the Search* / Fuse members of SIVO::ORBmatcher
 * (reference include/orbslam/ORBmatcher.h:44-120) from the PROJECTED point on:
 * window query on the frame grid (Frame::GetFeaturesInArea, Frame.cc:326-390),
 * the per-candidate gates, best / second-best Hamming scan, acceptance rule,
 * the dependence of every iteration on the matches made by the earlier
 * iterations of the same call, and the 30-bin rotation histogram
 * (ComputeThreeMaxima, ORBmatcher.cc:1545-1577) — all on the GPU.  What needs
 * the SLAM object graph stays with the caller and arrives as arrays
 * (MapPoint::isBad / Observations / PredictScale / GetDescriptor, the cv::Mat
 * pose algebra, the DBoW2 node lists).
 *
 * The reference loops are sequential: iteration i skips the keypoints that
 * iterations < i matched.  The device reproduces exactly that result by
 * speculation + repair: every query matches in parallel against the state the
 * call started with; if two accepted queries chose one keypoint, rounds repeat
 * in which query i sees the picks of the queries < i of the previous round,
 * until nothing changes (query i is final after round i at the latest; one
 * round when there is no collision).
 * ------------------------------------------------------------------------ */
typedef struct sivo_mframe *sivo_mframe_t;
/* The part of Frame / KeyFrame the matcher reads: mvKeysSemantic, mvRight (NULL =
 * monocular, all -1), mDescriptorsSemantic (n x 32), image bounds mnMinX .. mnMaxY,
 * mvScaleFactors / mvLevelSigma2 / mvInvLevelSigma2.  Builds mGrid
 * (AssignFeaturesToGrid, Frame.cc:205-221; 64 x 48 cells) and uploads everything. */
int sivo_mframe_create(const SivoKeyPoint *keys, int n, const float *u_right, const uint8_t *descriptors,
                       float min_x, float max_x, float min_y, float max_y, const float *scale_factors,
                       const float *level_sigma2, const float *inv_level_sigma2, int nlevels, int device,
                       sivo_mframe_t *out);
int sivo_mframe_destroy(sivo_mframe_t h);
/* The size of the device slab that holds the frame's arrays and the scratch of its searches.  A search that needs more moves the
 * frame to a bigger slab; tests read this to see that one did. */
int sivo_mframe_slab_bytes(sivo_mframe_t h, int64_t *bytes);
/* Frame::GetFeaturesInArea (Frame.cc:326-390) from that grid, host side, in the reference's order. */
int sivo_mframe_features_in_area(sivo_mframe_t h, float x, float y, float r, int min_level, int max_level,
                                 int32_t *out, int capacity, int *n_out);

#define SIVO_Q_VALID 1   /* the iteration is not skipped by the per-point tests in front of the window query */
#define SIVO_Q_BLOCKS 2  /* an accepted match of this query makes the keypoint unavailable to later queries */
#define SIVO_Q_STEREO 4  /* SearchForTriangulation: bStereo1 */
typedef struct {
    float u, v;            /* window centre (projected point; kp1.pt for SearchForTriangulation) */
    float radius;          /* GetFeaturesInArea r */
    int32_t lvl_lo, lvl_hi;/* admissible octaves lvl_lo <= octave <= lvl_hi */
    float ur;              /* projection into the right image (gate 1 and 2) */
    float gate;            /* gate 1: max |ur - mvRight[k]| */
    float angle;           /* keypoint angle of the query (rotation histogram) */
    int32_t flags;         /* SIVO_Q_* */
} SivoSearchQuery;

typedef struct {
    int32_t th_dist;           /* accept iff best <= th_dist (accept_lt: best < th_dist) */
    int32_t accept_lt;
    int32_t ratio_mode;        /* 0 none; 1 reject iff octave(best) == octave(second) && best > nn_ratio * second
                                  (ORBmatcher.cc:117-119); 2 accept only iff (float) best < nn_ratio * (float) second (:230, :582) */
    float nn_ratio;
    int32_t gate_mode;         /* 0 none; 1 skip k iff mvRight[k] > 0 && |ur - mvRight[k]| > gate (:93-97, :1353-1358);
                                  2 Fuse chi2: stereo 7.8 / mono 5.99 on the reprojection error (:880-902);
                                  3 SearchForTriangulation: dist <= th_dist, epipole distance, CheckDistEpipolarLine (:703-719) */
    int32_t check_orientation; /* mbCheckOrientation */
    int32_t dynamic;           /* later queries see earlier matches (sequential semantics) */
    int32_t tie_last;          /* 0: the first candidate wins ties (dist < best); 1: the last (:703 `dist > bestDist` continue) */
    float F12[9];              /* gate 3: fundamental matrix, row-major */
    float ex, ey;              /* gate 3: epipole in the train image */
} SivoSearchRule;

/* The engine.  Candidates of query q: the window query on the train frame's grid when cand_idx is NULL, else the
 * rows cand_idx[cand_begin[q] .. cand_end[q]) (BoW node lists; several queries may share a range).
 * blocked (n bytes, may be NULL): keypoints unavailable from the start.
 * Outputs (any may be NULL): match_query[q] = the keypoint query q is matched with after the rotation check, -1 none;
 * match_train[k] = the query whose match the call leaves in slot k (-1 untouched, -2 cleared by the rotation
 * check); best_dist / second_dist per query (256 = none); *n_matches as the reference routine counts it. */
int sivo_search(sivo_mframe_t train, const SivoSearchQuery *queries, const uint8_t *query_desc, int n_queries,
                const int32_t *cand_begin, const int32_t *cand_end, const int32_t *cand_idx, int n_cand,
                const SivoSearchRule *rule, const uint8_t *blocked, int32_t *match_query, int32_t *match_train,
                int32_t *best_dist, int32_t *second_dist, int *n_matches, int *rounds);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &, th)  (ORBmatcher.cc:44-127).
 * Per map point: track_in_view = mbTrackInView && !isBad(); proj_x / proj_y / proj_xr / level / view_cos = the
 * mTrack* fields; mp_desc = GetDescriptor(); mp_obs = Observations().  occ_obs[k] (in/out) = -1 where
 * F.mvpMapPoints[k] is NULL, else that point's Observations(); match[k] (out) = the map point stored into
 * F.mvpMapPoints[k], -1 where the call stored nothing. */
int sivo_search_by_projection_mappoints(sivo_mframe_t F, int n_mp, const uint8_t *track_in_view, const float *proj_x,
                                        const float *proj_y, const float *proj_xr, const int32_t *level,
                                        const float *view_cos, const uint8_t *mp_desc, const int32_t *mp_obs, float th,
                                        float nn_ratio, int32_t *occ_obs, int32_t *match, int *n_matches);
/* ORBmatcher::SearchByProjection(Frame &Current, const Frame &Last, th, bMono)  (ORBmatcher.cc:1278-1418).
 * Per last-frame key: valid = map point present && !mvbOutlier; u, v, inv_z = its projection with the current pose
 * (:1309-1322); last_octave / last_angle; mp_desc; mp_obs.  forward / backward = bForward / bBackward (:1299-1300).
 * match[k]: >= 0 last-frame key, -2 cleared by the rotation check, -1 untouched. */
int sivo_search_by_projection_frame(sivo_mframe_t current, int n_last, const uint8_t *valid, const float *u, const float *v,
                                    const float *inv_z, const int32_t *last_octave, const float *last_angle,
                                    const uint8_t *mp_desc, const int32_t *mp_obs, float th, int forward, int backward,
                                    float bf, int check_orientation, int32_t *occ_obs, int32_t *match, int *n_matches);
/* ORBmatcher::SearchByProjection(Frame &Current, KeyFrame*, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1420-1543).
 * valid = pMP && !isBad && !sAlreadyFound && distance inside the scale-invariance range; occupied[k] (in/out). */
int sivo_search_by_projection_reloc(sivo_mframe_t current, int n_kf, const uint8_t *valid, const float *u, const float *v,
                                    const int32_t *pred_level, const float *kf_angle, const uint8_t *mp_desc, float th,
                                    int orb_dist, int check_orientation, uint8_t *occupied, int32_t *match, int *n_matches);
/* ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)  (ORBmatcher.cc:286-399). */
int sivo_search_by_projection_kf(sivo_mframe_t kf, int n_mp, const uint8_t *valid, const float *u, const float *v,
                                 const int32_t *pred_level, const uint8_t *mp_desc, int th, uint8_t *matched,
                                 int32_t *match, int *n_matches);
/* ORBmatcher::Fuse (ORBmatcher.cc:787-929; scw_variant != 0: :931-1053): best_idx[i] = the keypoint map point i is
 * fused with (-1: none / bestDist > TH_LOW); the Replace / AddObservation surgery (:909-923) is the caller's. */
int sivo_fuse(sivo_mframe_t kf, int n_mp, const uint8_t *valid, const float *u, const float *v, const float *ur,
              const int32_t *pred_level, const uint8_t *mp_desc, float th, int scw_variant, int32_t *best_idx,
              int32_t *best_dist, int *n_fused);
/* ORBmatcher::SearchBySim3, one direction (ORBmatcher.cc:1102-1176 / :1178-1252): match_out[i] = best key or -1. */
int sivo_search_by_sim3_dir(sivo_mframe_t kf, int n, const uint8_t *valid, const float *u, const float *v,
                            const int32_t *pred_level, const uint8_t *mp_desc, float th, int32_t *match_out);
/* The BoW-guided routines.  DBoW2 is outside this library: the vocabulary nodes both operands hold arrive as two CSR
 * lists (node k: keys idx1[off1[k] .. off1[k+1]) of the first operand, idx2[off2[k] .. off2[k+1]) of the second).
 * SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:161-284): match_f[k] = keyframe key or -1. */
int sivo_search_by_bow_kf_frame(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                                const int32_t *idx2, const uint8_t *kf_valid, const SivoKeyPoint *keys_kf,
                                const uint8_t *desc_kf, int n_kf, sivo_mframe_t frame, float nn_ratio,
                                int check_orientation, int32_t *match_f, int *n_matches);
/* SearchByBoW(KeyFrame*, KeyFrame*, ...) (ORBmatcher.cc:508-629): matches12[idx1] = idx2 or -1. */
int sivo_search_by_bow_kf_kf(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                             const int32_t *idx2, const uint8_t *valid1, const SivoKeyPoint *keys1, const uint8_t *desc1,
                             int n1, const uint8_t *valid2, sivo_mframe_t kf2, float nn_ratio, int check_orientation,
                             int32_t *matches12, int *n_matches);
/* SearchForTriangulation (ORBmatcher.cc:631-785): F12 row-major, (ex, ey) the epipole in image 2. */
int sivo_search_for_triangulation(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                                  const int32_t *idx2, const SivoKeyPoint *keys1, const float *u_right1,
                                  const uint8_t *has_mp1, const uint8_t *desc1, int n1, sivo_mframe_t kf2,
                                  const uint8_t *has_mp2, const float F12[9], float ex, float ey, int only_stereo,
                                  int check_orientation, int32_t *matches12, int *n_matches);

/* Frame::ComputeStereoMatches (reference src/orbslam/Frame.cc:444-629):
 * row-band candidates, octave +-1, disparity window, best Hamming < 100,
 * accept < 75, 11x11 SAD slide +-5 on the pyramid level, parabola, median
 * cull.  Left/right keypoints and descriptors are host arrays; the pyramids
 * are those of two sivo_orb handles' last extraction (still in HBM).
 * u_right / depth: n_left floats, -1 where unmatched. */
/* sivo_stereo_match: a left or right key whose octave is outside [0, nlevels) of the extractors -> SIVO_ERR_INVALID_ARGUMENT, no output written. */
int sivo_stereo_match(sivo_orb_t left, sivo_orb_t right, const SivoKeyPoint *kp_left, const uint8_t *desc_left,
                      int n_left, const SivoKeyPoint *kp_right, const uint8_t *desc_right, int n_right,
                      float bf, float b, float *u_right, float *depth, int32_t *best_right);
/* The same in two steps, so that everything except the median cull (Frame.cc:616-628) can run while the network
 * is still computing the class map that SelectSemanticKeys (Frame.cc:177-203) needs: `begin` matches EVERY left
 * keypoint (each is independent of the other left keypoints) and returns the pre-cull u_right / depth plus the
 * SAD distance of each match (sad_dist, -1 where unmatched); `cull` then applies the median test over the
 * keypoints with keep[i] != 0 (NULL = all) and clears the others.  begin + cull(keep) == sivo_stereo_match on
 * the kept subset. */
/* sivo_stereo_match_begin: the keys' octaves are scanned first; one outside [0, nlevels) -> SIVO_ERR_INVALID_ARGUMENT, no output written. */
int sivo_stereo_match_begin(sivo_orb_t left, sivo_orb_t right, const SivoKeyPoint *kp_left, const uint8_t *desc_left,
                            int n_left, const SivoKeyPoint *kp_right, const uint8_t *desc_right, int n_right,
                            float bf, float b, float *u_right, float *depth, int32_t *best_right, int32_t *sad_dist);
int sivo_stereo_match_cull(int n, const uint8_t *keep, const int32_t *sad_dist, float *u_right, float *depth);

/* ===========================================================================
 * Bundle-adjustment edges — stands behind the g2o edges SIVO::Optimizer
 * builds (reference src/orbslam/Optimizer.cc:318-409, 651-755):
 * EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (+OnlyPose) computeError and
 * linearizeOplus, chi2 and the Huber kernel.
 * ======================================================================== */
typedef struct {
    int32_t pose;   /* index into poses: 12 doubles each, R row-major then t (world -> camera) */
    int32_t point;  /* index into points: 3 doubles each */
    int32_t stereo; /* 0 = (u,v), 1 = (u,v,uR) */
    int32_t pad_;
    double obs[3];
    double inv_sigma2; /* information = inv_sigma2 * I (Optimizer.cc:691-692, 730-733) */
} SivoEdge;

/* Per edge e: err[3e..] (err[2] = 0 for mono), Jx[9e..] 3x3 row-major
 * d err/d point, Jp[18e..] 3x6 row-major d err/d pose (rotation columns
 * first), chi2, rho (Huber-robustified chi2), w (Huber weight), depth_ok (z>0).
 * intr = {fx, fy, cx, cy, bf}. Any output pointer may be NULL. */
int sivo_ba_linearize_dev(const double *d_poses, const double *d_points, const SivoEdge *d_edges,
                          int64_t n_edges, const double intr[5], double delta_mono, double delta_stereo,
                          double *d_err, double *d_jx, double *d_jp, double *d_chi2, double *d_rho,
                          double *d_w, uint8_t *d_depth_ok, void *stream);
int sivo_ba_linearize(const double *poses, int n_poses, const double *points, int n_points,
                      const SivoEdge *edges, int64_t n_edges, const double intr[5], double delta_mono,
                      double delta_stereo, double *err, double *jx, double *jp, double *chi2, double *rho,
                      double *w, uint8_t *depth_ok);

/* ---------------------------------------------------------------------------
 * The optimisation loops g2o runs for SIVO::Optimizer, on arrays.
 * Levenberg-Marquardt as g2o::OptimizationAlgorithmLevenberg over BlockSolver_6_3:
 * robustified normal equations, landmark block marginalised by a Schur complement,
 * lambda_0 = 1e-5 max|diag H|, <= 10 trials per iteration, VertexSE3Expmap /
 * VertexSBAPointXYZ updates (restated in oracle/ba_solve_oracle.c).  Host arrays
 * in/out; every kernel runs on the GPU, the host only takes the accept/reject
 * decision of each trial (3 doubles back per trial).
 * ------------------------------------------------------------------------ */

/* One g2o `optimizer.optimize(iterations)` call — what Optimizer::BundleAdjustment
 * (Optimizer.cc:49-271) runs.  pose_fixed[i] != 0: keyframe i is held fixed
 * (setFixed, :73, :601-610).  level[e] != 0: edge excluded (setLevel(1));
 * robust[e] != 0: Huber kernel with delta_mono / delta_stereo; NULL = all
 * active / all robust.  At most one edge per (keyframe, map point) pair.
 * stop_flag (one byte, i.e. the reference's `bool *pbStopFlag`; may be NULL) is
 * polled between trials like g2o's forceStopFlag (:573-575).  poses and points are
 * updated in place; err_out (3 per edge, may be NULL) receives the error vectors
 * g2o would hold afterwards; hpp_last_out (36 per free pose, may be NULL) the
 * pose blocks of the last buildSystem. */
int sivo_ba_optimize(double *poses, const uint8_t *pose_fixed, int n_poses, double *points, int n_points,
                     const SivoEdge *edges, int64_t n_edges, const double intr[5], double delta_mono,
                     double delta_stereo, const uint8_t *level, const uint8_t *robust, int iterations,
                     const volatile uint8_t *stop_flag, double *err_out, double *hpp_last_out,
                     int *iterations_run, int *trials);

/* Optimizer::LocalBundleAdjustment from the point the graph is built
 * (Optimizer.cc:757-926): optimize(5) with Huber kernels; unless stopped, edges
 * with chi2 > 5.991 (mono) / 7.815 (stereo) or non-positive depth are excluded
 * and every kernel is dropped, optimize(10); outlier[e] = 1 for the observations
 * the caller must erase (:824-858).  cov (36, row-major) = the marginal block
 * of keyframe `cov_pose` as g2o's computeMarginals returns it (:900-907);
 * *cov_ok = 0 when that keyframe is fixed / out of range / its block is singular. */
int sivo_local_ba(double *poses, const uint8_t *pose_fixed, int n_poses, double *points, int n_points,
                  const SivoEdge *edges, int64_t n_edges, const double intr[5], const volatile uint8_t *stop_flag,
                  uint8_t *outlier, int cov_pose, double *cov, int *cov_ok, int *iterations, int *trials);

/* How the reduced camera system of a bundle adjustment is solved.  DENSE: a dense
 * (free pose x point) edge table, one workgroup per keyframe pair, a dense Cholesky
 * — the form of the local BA; refuses n_free * n_points > 2^28.  SPARSE: S holds
 * the blocks of keyframe pairs that share a point, is assembled from per-block
 * contribution lists and factored by a 6 x 6 block sparse Cholesky over a host
 * plan (minimum-degree order, elimination-tree levels) — the form of the global
 * BA.  AUTO: SPARSE when DENSE would refuse the problem or from 64 free keyframes
 * on, DENSE otherwise.  Zero-initialise, set size = sizeof(SivoBaOptions); NULL
 * means AUTO.  The library reads no environment variable. */
#define SIVO_BA_SOLVER_AUTO 0
#define SIVO_BA_SOLVER_DENSE 1
#define SIVO_BA_SOLVER_SPARSE 2
typedef struct SivoBaOptions {
    uint32_t size;               /* sizeof(SivoBaOptions) of the caller's header */
    int32_t solver;              /* SIVO_BA_SOLVER_* */
} SivoBaOptions;

/* sivo_ba_optimize / sivo_local_ba with options (NULL: the plain functions). */
int sivo_ba_optimize_opts(double *poses, const uint8_t *pose_fixed, int n_poses, double *points, int n_points,
                          const SivoEdge *edges, int64_t n_edges, const double intr[5], double delta_mono,
                          double delta_stereo, const uint8_t *level, const uint8_t *robust, int iterations,
                          const volatile uint8_t *stop_flag, double *err_out, double *hpp_last_out,
                          int *iterations_run, int *trials, const SivoBaOptions *opts);
int sivo_local_ba_opts(double *poses, const uint8_t *pose_fixed, int n_poses, double *points, int n_points,
                       const SivoEdge *edges, int64_t n_edges, const double intr[5], const volatile uint8_t *stop_flag,
                       uint8_t *outlier, int cov_pose, double *cov, int *cov_ok, int *iterations, int *trials,
                       const SivoBaOptions *opts);

/* What the host prepares for the sparse path of a problem, without touching a
 * device: out[0] free poses, [1] blocks of S below the diagonal, [2] off-diagonal
 * blocks of L, [3] nnz(L) in scalars (lower triangle), [4] flops of one numeric
 * factorisation, [5] levels of the elimination tree, [6] contribution pairs,
 * [7] the path `opts` takes (1 dense, 2 sparse).  An index out of range, two
 * edges on one (keyframe, map point) pair, a NULL array with a non-zero count, or
 * DENSE on a problem the dense path refuses -> SIVO_ERR_INVALID_ARGUMENT. */
int sivo_ba_analyze(const uint8_t *pose_fixed, int n_poses, int n_points, const SivoEdge *edges, int64_t n_edges,
                    const SivoBaOptions *opts, int64_t out[8]);

/* Optimizer::PoseOptimization from the point the edges are built
 * (Optimizer.cc:409-491): 4 rounds of optimize(10) from the initial pose, chi2
 * test (7.815) on the STEREO edges after each round — the reference never
 * re-classifies the mono edges (:432-467) — kernels of the stereo edges dropped
 * after the third round, pose + 6x6 covariance out.  edges[e].pose is ignored;
 * edges[e].point indexes `points` (map-point world positions, held fixed).
 * outlier (n_edges) = Frame::mvbOutlier; *n_inliers = nInitialCorrespondences -
 * nBad (0 and pose_out = pose0 when n_edges < 3, :409-411).  The whole schedule is
 * one launch of one persistent workgroup. */
int sivo_pose_optimize(const double pose0[12], const double *points, int n_points, const SivoEdge *edges,
                       int64_t n_edges, const double intr[5], uint8_t *outlier, double pose_out[12],
                       double cov[36], int *cov_ok, double *chi2, int *n_inliers, int *iterations,
                       int *trials);

/* ---------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 from the point the graph is built (Optimizer.cc:1236-1449):
 * one VertexSim3Expmap against EdgeSim3ProjectXYZ + EdgeInverseSim3ProjectXYZ per
 * correspondence (points held fixed, g2o's numeric Jacobians), Huber kernels with
 * delta = sqrtf(th2); optimize(5), a pair is an outlier if either chi2 > th2; fewer
 * than 10 survivors -> *n_inliers = 0 and s12 unchanged (the flags of that test
 * stay set); else optimize(10) if a pair was removed, optimize(5) if not, final
 * test.  The whole schedule is one launch of one persistent workgroup per problem.
 * ------------------------------------------------------------------------ */
typedef struct {
    double obs1[2], inv_sigma2_1; /* keypoint of KF1 (mvKeysSemantic[i]), mvInvLevelSigma2[octave] */
    double obs2[2], inv_sigma2_2; /* keypoint of KF2 (mvKeysSemantic[i2]) */
    double x1c[3], x2c[3];        /* map points in camera-1 / camera-2 coordinates (held fixed) */
} SivoSim3Match;

/* s12[8] in/out: qx qy qz qw tx ty tz s (g2o's Sim3 state).  k1, k2 = {fx, fy, cx, cy}.
 * outlier[i] = 1: the pair the reference drops from vpMatches1.  chi2_12 / chi2_21: the
 * chi2 of the two edges the last test read (a pair removed by the first test keeps the
 * values of that test).  iterations / trials: LM iterations and trials of both
 * optimize() calls.  Every output pointer other than s12 and n_inliers may be NULL. */
int sivo_sim3_optimize(double s12[8], const double k1[4], const double k2[4], const SivoSim3Match *m, int n,
                       float th2, int fix_scale, uint8_t *outlier, int *n_inliers, double *chi2_12,
                       double *chi2_21, int *iterations, int *trials);

/* One problem of sivo_sim3_optimize_batch: the arguments of sivo_sim3_optimize (s12 in/out),
 * the three counts out. */
typedef struct {
    double s12[8], k1[4], k2[4];
    const SivoSim3Match *matches;
    int32_t n;
    float th2;
    int32_t fix_scale;
    int32_t n_inliers;            /* out */
    uint8_t *outlier;             /* n, may be NULL */
    double *chi2_12, *chi2_21;    /* n each, may be NULL */
    int32_t iterations, trials;   /* out */
} SivoSim3Problem;

/* n_problems independent problems (every loop candidate at once) in one launch, one
 * workgroup each: every result is bit-identical to sivo_sim3_optimize on that problem. */
int sivo_sim3_optimize_batch(SivoSim3Problem *problems, int n_problems);

/* ---------------------------------------------------------------------------
 * Sim3Solver's RANSAC (Sim3Solver.cc), the step of LoopClosing::ComputeSim3 in front
 * of OptimizeSim3: every hypothesis of every loop candidate in one launch.  Per
 * hypothesis: Horn's closed form on the three sampled pairs (ComputeSim3, :224-349),
 * then CheckInliers (:352-372) over all pairs: a pair is an inlier when both squared
 * reprojection errors (Project, :387-409, against FromCameraToImage, :411-429) are
 * below its thresholds.  CV_32F arithmetic with OpenCV's rounding; cv::eigen is a
 * fixed-sweep cyclic Jacobi in double and atan2 + cv::Rodrigues the rotation matrix of
 * the quaternion.  Results are bit-identical run to run and between the
 * single and the batched call.
 * ------------------------------------------------------------------------ */
typedef struct {
    float x1c[3], x2c[3];         /* mvX3Dc1[i], mvX3Dc2[i] (:96, :99) */
    float max_err1, max_err2;     /* (float) mvnMaxError1[i], mvnMaxError2[i]: (unsigned long)(9.210 * sigma2) (:86-89) */
} SivoSim3Pair;                   /* 32 bytes */

typedef struct {
    const SivoSim3Pair *pairs;
    int32_t n;
    float k1[4], k2[4];           /* fx fy cx cy */
    const int32_t *triples;       /* 3 n_hyp indices into pairs, as drawn (:166-180) */
    int32_t n_hyp;
    int32_t min_inliers, fix_scale;
    /* out, all caller-owned: */
    int32_t *count;               /* n_hyp: mnInliersi of each hypothesis */
    float *T;                     /* 13 n_hyp: R12 row-major, t12, s12 (mR12i, mt12i, ms12i); a NaN is stored as 0x7FC00000 */
    uint64_t *inlier_bits;        /* n_hyp * ceil(n / 64) words, bit p%64 of word p/64 = mvbInliersi[p] */
    int32_t first_accept, best;   /* first h with count > min_inliers (-1: none); last h attaining the running
                                   * maximum under >= (:186-200; -1 without hypotheses) */
} SivoSim3RansacProblem;

/* A triple index out of range or repeated inside a triple, n < 3 with n_hyp > 0, or a NULL
 * array with a non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched.
 * n_problems == 0, or n_hyp == 0 everywhere: no launch. */
int sivo_sim3_ransac_batch(SivoSim3RansacProblem *problems, int n_problems);
/* The batch of one. */
int sivo_sim3_ransac(SivoSim3RansacProblem *problem);

/* ---------------------------------------------------------------------------
 * PnPsolver's EPnP RANSAC (PnPsolver.cc), the step of Tracking::Relocalization
 * (Tracking.cc:1279-1330) between SearchByBoW and PoseOptimization: every hypothesis of
 * every candidate keyframe in one launch, then every Refine in a second one.  Per
 * hypothesis: compute_pose (:482-531) on the four sampled correspondences, then
 * CheckInliers (:318-347) over all of them.  A hypothesis is a RECORD when its count is
 * >= min_inliers and strictly above every earlier count and best_in: the iterations at
 * which iterate (:228-241) replaces mvbBestInliers.  Refine (:271-315) is a pure function
 * of mvbBestInliers, so only records are refined: compute_pose on the record's inliers,
 * CheckInliers again.  Arithmetic in double as the source has it; cvSVD / cvSolve /
 * cvInvert are a fixed-sweep Jacobi, the source's own qr_solve and the adjugate (DESIGN
 * 3.6d).  Results are bit-identical run to run and between the single and the batched call.
 * ------------------------------------------------------------------------ */
typedef struct {
    float xw[3];                  /* mvP3Dw[i] (:103) */
    float u, v;                   /* mvP2D[i] (:99) */
    float max_err;                /* mvMaxError[i] = mvSigma2[i] * th2 (:172) */
} SivoPnpPoint;                   /* 24 bytes */

typedef struct {
    const SivoPnpPoint *points;
    int32_t n;
    float K[4];                   /* fx fy cx cy */
    int32_t min_inliers;          /* mRansacMinInliers, >= 4 */
    int32_t best_in;              /* mnBestInliers on entry: 0 for a fresh solver */
    const int32_t *samples;       /* 4 n_hyp indices into points, as drawn (:203-220) */
    int32_t n_hyp;
    /* out, all caller-owned: */
    int32_t *count;               /* n_hyp: mnInliersi of each hypothesis */
    float *T;                     /* 12 n_hyp: mRi row-major, mti, converted CV_64F -> CV_32F (:234-237); a NaN is 0x7FC00000 */
    uint64_t *inlier_bits;        /* n_hyp * ceil(n / 64) words, bit p%64 of word p/64 = mvbInliersi[p] */
    int32_t *refined;             /* n_hyp: mnRefinedInliers of a record, -1 where the hypothesis is no record */
    float *refined_T;             /* 12 n_hyp: row h written where refined[h] >= 0 */
    uint64_t *refined_bits;       /* n_hyp * ceil(n / 64): row h written where refined[h] >= 0 (mvbRefinedInliers) */
    int32_t n_records;            /* out */
} SivoPnpRansacProblem;

/* A sample index out of range or repeated inside a sample, n < 4 or min_inliers < 4 with
 * n_hyp > 0, or a NULL array with a non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any
 * device is touched.  n_problems == 0, or n_hyp == 0 everywhere: no launch.  No record
 * anywhere: no second launch. */
int sivo_pnp_ransac_batch(SivoPnpRansacProblem *problems, int n_problems);
/* The batch of one. */
int sivo_pnp_ransac(SivoPnpRansacProblem *problem);

/* ---------------------------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph from the point the graph is built
 * (Optimizer.cc:928-1180: the graph of :964-1175, then optimize(20)): one
 * VertexSim3Expmap per keyframe, EdgeSim3 edges with information I7 and no robust
 * kernel, error = log(Sji * Si * Sj^-1) (g2o's Sim3::log), BaseBinaryEdge's numeric
 * Jacobians (central differences, delta = 1e-9, through oplus), Levenberg-Marquardt
 * with lambda_0 = 1e-16 (setUserLambdaInit) over the sparse 7n x 7n system.
 * The host orders the variables and factors the pattern symbolically once per call;
 * the device assembles H, factors H + lambda I by sparse block Cholesky, solves,
 * updates and takes every LM decision.  Results are bit-identical run to run.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t i, j;                 /* vertex 0 / vertex 1 of the EdgeSim3 (indices into siw) */
    double meas[8];               /* Sji: qx qy qz qw tx ty tz s */
} SivoSim3Edge;

/* siw[8 n] in/out: Siw of vertex k (qx qy qz qw tx ty tz s); fixed[n]: 1 = setFixed(true).
 * A vertex without edges, or fixed, keeps its estimate.  No edge, or no vertex both
 * free and on an edge: no iteration (g2o's optimize() returns at once).  fix_scale:
 * VertexSim3Expmap::_fix_scale (update[6] = 0).  chi2[2] (may be NULL): sum of e'e over
 * the edges at the input and at the returned estimate.  iterations_done / trials may
 * be NULL.  Index out of range, i == j, a non-positive scale or a NULL array with a
 * non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched. */
int sivo_essential_graph_optimize(double *siw, const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne,
                                  int fix_scale, int iterations, double *chi2, int *iterations_done,
                                  int *trials);

/* The host half of sivo_essential_graph_optimize on its own (no device): the ordering
 * and symbolic factorisation it would use.  out[6]: variables (free vertices on an
 * edge), block columns of L that are not diagonal, nnz(L) in scalars (lower triangle),
 * flops of one numeric factorisation, levels of the elimination tree, pattern blocks
 * of H below the diagonal. */
int sivo_essential_graph_analyze(const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne, int64_t out[6]);

/* The map-point correction of OptimizeEssentialGraph (Optimizer.cc:1205-1233):
 * out[k] = (float) correctedSwr.map(Srw.map((double) xyz[k])) with Srw = siw_before[r],
 * correctedSwr = siw_after[r]^-1, r = ref[k]; ref[k] = -1: out[k] = xyz[k].  xyz, out:
 * 3 np floats (may alias). */
int sivo_sim3_correct_points(const float *xyz, const int32_t *ref, int np, const double *siw_before,
                             const double *siw_after, int n, float *out);

/* ===========================================================================
 * Entropy feature-selection gate (the Tracking form; sivo_check_semantics below is the LocalMapping form) — stands behind SIVO's sivo_helpers
 * (reference src/sivo_helpers/sivo_helpers.cpp:64-88 computeStereoJacobianPose,
 * :160-180 computeStereoCovariance, :201-219 computeStereoMutualInformation) as
 * Tracking::CreateNewKeyFrame applies them per semantic keypoint
 * (reference src/orbslam/Tracking.cc:934-1023).  SURVEY.md 8f-1.
 * For keypoint i: skip unless depth[i] > 0; J = stereo pose Jacobian at
 * xyz[3i..] (the coordinates the caller passes — the reference passes WORLD
 * coordinates, Tracking.cc:963-977); S9 = [[Sx, Sx J'],[J Sx, J Sx J' + sigma2 I]];
 * MI = 0.5 log2(det Sx * det Sz / det S9); reduction = MI - entropy(row, col) at
 * the truncated keypoint position; accept iff reduction > th.
 * state_cov: 6x6 row-major (Frame::mSigmacw); level_sigma2: mvLevelSigma2.
 * ======================================================================== */
/* sivo_entropy_gate_dev: the keys are on the device and are not scanned; a key whose octave is outside [0, nlevels) fails the gate
 * (MI 0, reduction 0, accept 0) and level_sigma2 is not indexed with it. */
int sivo_entropy_gate_dev(int n, const SivoKeyPoint *d_kps, const float *d_depth, const double *d_xyz,
                          const double *d_entropy, int rows, int cols, const double state_cov[36], double fx,
                          double fy, double bl, const float *level_sigma2, int nlevels, double th,
                          double *d_mi, double *d_reduction, uint8_t *d_accept, void *stream);
/* Host key arrays against the DEVICE-resident entropy map (what sivo_segnet_segment_dev left in HBM): the form the per-frame
 * path uses — the keys come out of the semantic filter on the host, the map stays where the network wrote it.  Synchronous;
 * the caller has synchronised with the producer of d_entropy. */
/* sivo_entropy_gate_map_dev: an octave outside [0, nlevels) -> SIVO_ERR_INVALID_ARGUMENT before anything is staged, outputs untouched. */
int sivo_entropy_gate_map_dev(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz,
                              const double *d_entropy, int rows, int cols, const double state_cov[36], double fx,
                              double fy, double bl, const float *level_sigma2, int nlevels, double th, double *mi,
                              double *reduction, uint8_t *accept);
/* sivo_entropy_gate: an octave outside [0, nlevels) -> SIVO_ERR_INVALID_ARGUMENT before anything is staged, outputs untouched. */
int sivo_entropy_gate(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz,
                      const double *entropy, int rows, int cols, const double state_cov[36], double fx,
                      double fy, double bl, const float *level_sigma2, int nlevels, double th, double *mi,
                      double *reduction, uint8_t *accept);

/* LocalMapping::CheckSemantics(pKF, idx, wP, compute_information = true) (reference src/orbslam/LocalMapping.cc:474-538)
 * over n keypoints: detected_class[i] = the class at the truncated keypoint position if depth > 0, the class is static
 * (<= TERRAIN = 8), confidence >= th_confidence and NOT (MI - entropy < th_entropy) — equality passes, unlike the
 * Tracking gate above — else VOID (255).  mi / reduction may be NULL. */
/* sivo_check_semantics_dev: a key whose octave is outside [0, nlevels) fails (MI 0, reduction 0, class VOID), nothing is indexed with it. */
int sivo_check_semantics_dev(int n, const SivoKeyPoint *d_kps, const float *d_depth, const double *d_xyz,
                             const double *d_entropy, const double *d_confidence, const uint8_t *d_classes, int rows, int cols,
                             const double state_cov[36], double fx, double fy, double bl, const float *level_sigma2,
                             int nlevels, double th_entropy, double th_confidence, double *d_mi, double *d_reduction,
                             uint8_t *d_detected_class, void *stream);
/* sivo_check_semantics: an octave outside [0, nlevels) -> SIVO_ERR_INVALID_ARGUMENT before anything is staged, outputs untouched. */
int sivo_check_semantics(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz, const double *entropy,
                         const double *confidence, const uint8_t *classes, int rows, int cols, const double state_cov[36],
                         double fx, double fy, double bl, const float *level_sigma2, int nlevels, double th_entropy,
                         double th_confidence, double *mi, double *reduction, uint8_t *detected_class);

/* ===========================================================================
 * LocalMapping::CreateNewMapPoints, the body of the loop over the matches
 * (reference src/orbslam/LocalMapping.cc:277-470) for ONE keyframe pair: the
 * parallax test (:289-319), the linear triangulation (:320-338) or the stereo
 * unprojection (:340-343, KeyFrame.cc:642-656), the depth tests (:351-362), the
 * reprojection tests (:364-425), the scale-consistency test (:427-446) and both
 * CheckSemantics calls (:449-452, :474-545).  One thread per match.  Float
 * arithmetic as OpenCV 3.x does it (api/compat/cv_min.hpp); two pieces are
 * restated, not pinned: the null vector of A (cv::SVD::compute) is
 * the eigenvector of the smallest eigenvalue of A'A by cyclic Jacobi in double, and
 * cos(2 atan2(mb / 2, depth)) is (d^2 - a^2) / (d^2 + a^2) in double.
 * Results are bit-identical run to run and between the single and the batched call.
 * ======================================================================== */
typedef struct {
    float Rcw[9], tcw[3];         /* GetRotation(), GetTranslation() (:210-212, :261-263) */
    float Ow[3];                  /* GetCameraCenter() (:216, :238) */
    float Twc[12];                /* mTwc.rowRange(0, 3), row-major 3 x 4 (KeyFrame.cc:652) */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    int32_t nlevels;              /* mnScaleLevels, 1 .. 16 */
    float scale_factors[16];      /* mvScaleFactors */
    float level_sigma2[16];       /* mvLevelSigma2 */
} SivoTriKeyFrame;                /* 272 bytes */

typedef struct {
    float x1, y1;                 /* mvKeysSemantic[idx1].pt of the current keyframe (:281) */
    int32_t octave1;
    float r1, depth1;             /* mvRight[idx1] (< 0: no stereo), mvDepth[idx1] */
    float x2, y2;                 /* the same of the neighbour (:285-286) */
    int32_t octave2;
    float r2, depth2;
    double entropy1, confidence1; /* mEntropy / mConfidence of keyframe 1 at ((int) y1, (int) x1) (:479-484) */
    uint8_t class1, class2;       /* mClasses of keyframe 1 / keyframe 2 at the truncated keypoint positions (:485) */
    uint8_t pad_[6];
} SivoTriMatch;                   /* 64 bytes */

enum {
    SIVO_TRI_ACCEPTED = 0,
    SIVO_TRI_LOW_PARALLAX = 1,    /* :344-347 */
    SIVO_TRI_W_ZERO = 2,          /* :333-335 */
    SIVO_TRI_Z1 = 3,              /* :354-356 */
    SIVO_TRI_Z2 = 4,              /* :360-362 */
    SIVO_TRI_REPROJ1 = 5,         /* :378-380, :388-391 */
    SIVO_TRI_REPROJ2 = 6,         /* :409-411, :421-424 */
    SIVO_TRI_ZERO_DIST = 7,       /* :434-436 */
    SIVO_TRI_SCALE = 8,           /* :443-446 */
    SIVO_TRI_SEMANTICS = 9        /* :452 */
};

typedef struct {
    SivoTriKeyFrame kf1, kf2;     /* mpCurrentKeyFrame, pKF2 */
    float ratio_factor;           /* 1.5f * mfScaleFactor (:225) */
    int32_t pad_;
    double state_cov[36];         /* keyframe 1: GetCovariance(), row-major */
    double th_confidence;         /* keyframe 1: mThConfidence */
    double th_entropy;            /* keyframe 1: mThEntropyReduction */
    const SivoTriMatch *matches;
    int32_t n;
    int32_t pad2_;
    /* out, caller-owned: */
    uint8_t *status;              /* n: SIVO_TRI_* — the `continue` that rejected the match */
    float *wP;                    /* 3 n: the point as it stood when the match left the loop (0 for status 1 and 2); a NaN is 0x7FC00000 */
    uint8_t *detected_class;      /* n: CheckSemantics(keyframe 1, ..., true) where the match reached it, else VOID (255) */
} SivoTriProblem;

/* An octave outside [0, nlevels), nlevels outside [1, 16], n < 0 or a NULL array with
 * n > 0 -> SIVO_ERR_INVALID_ARGUMENT before any device is touched.  n == 0 everywhere:
 * no launch. */
int sivo_triangulate(SivoTriProblem *problem);
/* Several keyframe pairs in one launch (a workgroup table). */
int sivo_triangulate_batch(SivoTriProblem *problems, int n_problems);

/* MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth
 * (reference src/orbslam/MapPoint.cc:284-347, :368-411) for np map points at once,
 * one wavefront per point.  Point p owns the descriptors desc[32 * desc_off[p] ..
 * 32 * desc_off[p + 1]) — vDescriptors in the order of the walk over mObservations,
 * bad keyframes left out (:305-310) — and the camera centres obs_ow[3 * obs_off[p] ..
 * 3 * obs_off[p + 1]) of ALL its observations (:391-397).
 * best_idx[p]: BestIdx (:330-341) — the first row of the N x N Hamming matrix whose
 * median, the element (int)(0.5 (N - 1)) of the sorted row, is strictly smallest.
 * max_dist / min_dist / normal[3 p]: mfMaxDistance, mfMinDistance, mNormalVector
 * (:399-409) from pos = mWorldPos, ref_ow = pRefKF->GetCameraCenter(), level_scale =
 * pRefKF->mvScaleFactors[level], last_scale = pRefKF->mvScaleFactors[nLevels - 1].
 * flags[p]: bit 0 = no observation (both functions return early, :299-301 / :385-387:
 * nothing of the point is written), bit 1 = no descriptor (:312-313: best_idx[p] is not
 * written).  A NaN is stored as 0x7FC00000.
 * np < 0, an offset array that does not start at 0 or decreases, or a NULL array with
 * a non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched. */
enum { SIVO_MP_NO_OBSERVATION = 1, SIVO_MP_NO_DESCRIPTOR = 2 };
int sivo_mappoint_refresh(int np, const int64_t *desc_off, const uint8_t *desc, const int64_t *obs_off, const float *obs_ow,
                          const float *pos, const float *ref_ow, const float *level_scale, const float *last_scale,
                          int32_t *best_idx, float *max_dist, float *min_dist, float *normal, uint8_t *flags);

/* ===========================================================================
 * Tracking::SearchLocalPoints (reference src/orbslam/Tracking.cc:1033-1085): the
 * local map culled with Frame::isInFrustum (Frame.cc:267-324, with
 * MapPoint::PredictScale, MapPoint.cc:439-453), then matched with
 * ORBmatcher::SearchByProjection(Frame &, const vector<MapPoint *> &, th).
 * One thread per map point; DESIGN 3.6g.
 * ======================================================================== */
typedef struct {
    float Rcw[9], tcw[3];          /* mTcw, row-major; mOw is derived from them */
    float fx, fy, cx, cy, bf;      /* bf = mbf */
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
    float log_scale_factor;        /* mfLogScaleFactor = logf(mfScaleFactor), > 0 */
    int32_t nlevels;               /* mnScaleLevels, 1 .. 16 */
    float cos_limit;               /* viewingCosLimit (Tracking passes 0.5) */
} SivoFrustum;                     /* 96 bytes */

enum {
    SIVO_FRUSTUM_IN_VIEW = 0,
    SIVO_FRUSTUM_BEHIND = 1,       /* Frame.cc:280 PcZ < 0 */
    SIVO_FRUSTUM_U = 2,            /* :288 u outside [mnMinX, mnMaxX] */
    SIVO_FRUSTUM_V = 3,            /* :290 v outside [mnMinY, mnMaxY] */
    SIVO_FRUSTUM_DISTANCE = 4,     /* :299 outside [0.8 min_dist, 1.2 max_dist] */
    SIVO_FRUSTUM_ANGLE = 5,        /* :308 viewCos < cos_limit */
    SIVO_FRUSTUM_SKIPPED = 6       /* skip[i] != 0: isBad() or mnLastFrameSeen == the frame's id (Tracking.cc:1057-1063) */
};

/* isInFrustum for n map points: pos = mWorldPos, normal = mNormalVector (3 n each),
 * min_dist / max_dist = mfMinDistance / mfMaxDistance (NOT the *Invariance getters:
 * the factors 0.8f and 1.2f are applied inside), skip (n bytes) may be NULL.
 * status[i] = SIVO_FRUSTUM_*, the `return false` the point took.  proj_x, proj_y,
 * proj_xr, view_cos and level receive mTrackProjX, mTrackProjY, mTrackProjXR,
 * mTrackViewCos and mnTrackScaleLevel of the points IN VIEW; the entries of every
 * other point are left as the caller had them.  *n_in_view = the number of status 0.
 * nlevels outside [1, 16], log_scale_factor <= 0, n < 0 or a NULL array with n > 0
 * -> SIVO_ERR_INVALID_ARGUMENT before any device is touched. */
int sivo_frustum_cull(const SivoFrustum *frustum, int n, const float *pos, const float *normal, const float *min_dist,
                      const float *max_dist, const uint8_t *skip, uint8_t *status, float *proj_x, float *proj_y,
                      float *proj_xr, float *view_cos, int32_t *level, int *n_in_view);
/* The same on device arrays (the frustum itself is a host struct), asynchronous on
 * `stream`; d_n_in_view (one int32 on the device) may be NULL. */
int sivo_frustum_cull_dev(const SivoFrustum *frustum, int n, const float *d_pos, const float *d_normal,
                          const float *d_min_dist, const float *d_max_dist, const uint8_t *d_skip, uint8_t *d_status,
                          float *d_proj_x, float *d_proj_y, float *d_proj_xr, float *d_view_cos, int32_t *d_level,
                          int32_t *d_n_in_view, void *stream);
/* The second loop of Tracking::SearchLocalPoints and the search behind it in one
 * call: the points travel in the search engine's one upload, a kernel culls them and
 * writes the query of every point in view on the device, and the engine's rounds run
 * on those.  mp_desc (32 n) = GetDescriptor(), mp_obs (n) = Observations(); th,
 * nn_ratio, occ_obs (in/out) and match (out) as sivo_search_by_projection_mappoints.
 * status (n) as sivo_frustum_cull; proj_x .. level may each be NULL and are written
 * for the points in view only.  *n_to_match = nToMatch (the points in view),
 * *n_matches = what SearchByProjection returns (0 when nothing is in view: the
 * reference then skips the search).  frustum->nlevels must not exceed the frame's. */
int sivo_search_local_points(sivo_mframe_t F, const SivoFrustum *frustum, int n, const float *pos, const float *normal,
                             const float *min_dist, const float *max_dist, const uint8_t *skip, const uint8_t *mp_desc,
                             const int32_t *mp_obs, float th, float nn_ratio, int32_t *occ_obs, int32_t *match,
                             uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos, int32_t *level,
                             int *n_to_match, int *n_matches);

/* ===========================================================================
 * ORBmatcher::Fuse for a list of map points into EVERY target keyframe in one call:
 * the loops of LocalMapping::SearchInNeighbors (reference LocalMapping.cc:586-594)
 * and LoopClosing::SearchAndFuse (LoopClosing.cc:609-635) up to the choice of the
 * keypoint.  The per-point tests of ORBmatcher.cc:814-852 / :966-1006 (projection,
 * image, distance, viewing angle, PredictScale) and the window query run on the
 * device, one wave per (keyframe, point) pair; the Replace / AddObservation surgery
 * is the caller's (SIVO::FuseIntoKeyFrames / SIVO::SearchAndFuse replay it in the
 * reference's order).  DESIGN 3.6k.
 * ======================================================================== */
typedef struct {
    float Rcw[9], tcw[3];             /* Tcw form: GetRotation / GetTranslation; Scw form: sRcw / s and t / s, as matcher_detail::Pose(Scw, s) */
    float Ow[3];                      /* Tcw form: GetCameraCenter() as stored; Scw form: -Rcw' tcw as Pose::centre */
    float fx, fy, cx, cy, bf;
    float min_x, max_x, min_y, max_y;
    float log_scale_factor;           /* > 0 */
    int32_t nlevels;                  /* 1 .. 16, not above the frame's */
    int32_t scw_variant;              /* as sivo_fuse's argument */
} SivoFuseCamera;                     /* 108 bytes */

enum { SIVO_FUSE_MATCHED = 0, SIVO_FUSE_SKIPPED, SIVO_FUSE_BEHIND, SIVO_FUSE_IMAGE, SIVO_FUSE_DISTANCE,
       SIVO_FUSE_ANGLE, SIVO_FUSE_NO_CANDIDATE, SIVO_FUSE_TOO_FAR };   /* the `continue` the pair took; TOO_FAR: bestDist > TH_LOW */

/* kfs / cams: n_kf frames and their cameras.  pos, normal (3 n_mp each), min_dist,
 * max_dist = mfMinDistance / mfMaxDistance (the factors 0.8f and 1.2f are applied
 * inside), mp_desc (32 n_mp).  skip_point[i] != 0: point i takes part in no pair;
 * skip_pair[k * n_mp + i] != 0: that pair is skipped (both may be NULL).
 * Outputs are row-major by keyframe: best_idx[k * n_mp + i] = the keypoint of
 * keyframe k that point i fuses with or -1, for every pair what sivo_fuse on keyframe
 * k gives for the host projection of that point; best_dist as sivo_fuse (256, resp.
 * INT_MAX in the Scw form, where no candidate was compared); status = SIVO_FUSE_*.
 * u, v, ur, level (each may be NULL) are written for the pairs that reach the window
 * query (status MATCHED, NO_CANDIDATE, TOO_FAR) and left alone otherwise.
 * Negative counts, a NULL required array with a positive count, a NULL frame, frames
 * on different devices, nlevels outside [1, 16] or above the frame's, or
 * log_scale_factor <= 0 -> SIVO_ERR_INVALID_ARGUMENT before any device is touched,
 * nothing written.  n_kf == 0 or n_mp == 0 succeeds and launches nothing.  Every
 * frame must be free of other calls for the duration (a frame serves one search at
 * a time); they are usable by sivo_fuse / sivo_search again when the call returns. */
int sivo_fuse_batch(const sivo_mframe_t *kfs, const SivoFuseCamera *cams, int n_kf, int n_mp,
                    const float *pos, const float *normal, const float *min_dist, const float *max_dist,
                    const uint8_t *mp_desc, const uint8_t *skip_point /* n_mp or NULL */,
                    const uint8_t *skip_pair /* n_kf * n_mp or NULL */, float th,
                    int32_t *best_idx, int32_t *best_dist, uint8_t *status,
                    float *u, float *v, float *ur, int32_t *level /* each n_kf * n_mp, each may be NULL */);

/* ===========================================================================
 * Covisibility bookkeeping: KeyFrame::UpdateConnections (reference
 * src/orbslam/KeyFrame.cc:327-415), the vote of Tracking::UpdateLocalKeyFrames
 * (Tracking.cc:1126-1142), LocalMapping::KeyFrameCulling (LocalMapping.cc:727-792)
 * and LocalMapping::MapPointCulling (LocalMapping.cc:165-196).  All four walk map
 * points and their observation lists; the work is integer and exact.  DESIGN 3.6h.
 * ======================================================================== */
typedef struct {
    int32_t n_kf;              /* keyframes are dense indices 0 .. n_kf-1 chosen by the caller */
    int32_t n_points;
    const int64_t *obs_off;    /* n_points + 1, CSR over mObservations */
    const int32_t *obs_kf;     /* keyframe index of each observation */
    const uint8_t *obs_level;  /* mvKeysSemantic[idx].octave of that observation */
    const uint8_t *obs_stereo; /* mvRight[idx] >= 0 (MapPoint.cc:157, :170) */
    const uint8_t *point_bad;  /* n_points: isBad() */
} SivoObsTable;

/* Above this many keyframes the count kernel's histogram no longer lives in LDS
 * (32 KiB of counters) and the kernel adds into the zeroed output row instead. */
#define SIVO_COVIS_LDS_KF 8192

/* The counting loop of KeyFrame::UpdateConnections (KeyFrame.cc:340-360) and of
 * Tracking::UpdateLocalKeyFrames (Tracking.cc:1129-1142) for n_sets slot lists in one
 * launch.  Set s is set_point[set_off[s] .. set_off[s + 1]): mvpMapPoints of one
 * keyframe or frame, -1 for a null slot.  counts[s * n_kf + k] = the number of slots
 * of the set whose point is not bad and is observed by keyframe k; observations by
 * k == set_self[s] are skipped (KeyFrame.cc:356), set_self[s] = -1 skips none
 * (Tracking.cc:1135-1137).  A point in two slots counts twice.  Every entry of
 * counts is written.
 * For this and the two calls below: an offset array that does not start at 0 or
 * that decreases, an index outside its range, a negative count or a NULL array with
 * a non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched; zero
 * work -> no launch. */
int sivo_covis_count(const SivoObsTable *t, int n_sets, const int64_t *set_off, const int32_t *set_point,
                     const int32_t *set_self, int32_t *counts);

enum {
    SIVO_KFCULL_KEPT = 0,
    SIVO_KFCULL_CULLED = 1,        /* SetBadFlag ran: the keyframe's observations left every point (KeyFrame.cc:493-495) */
    SIVO_KFCULL_TO_BE_ERASED = 2,  /* SetBadFlag on a keyframe with mbNotErase (KeyFrame.cc:482-485): nothing changes */
    SIVO_KFCULL_ID0 = 3            /* LocalMapping.cc:735 */
};

/* The whole loop of LocalMapping::KeyFrameCulling (LocalMapping.cc:732-791) over
 * n_local keyframes in the caller's order, in one launch, with the reference's
 * sequential effects: a culled, erasable keyframe's observations are removed from
 * every point (MapPoint.cc:164-189: nObs falls by 2 for a stereo observation, else by
 * 1; a point whose nObs is <= 2 after such a removal is bad from then on and later
 * keyframes skip it).  Observations() of :757 is the weighted sum over the
 * observations that are left.
 * Local keyframe j: local_kf[j] its table index, is_id0[j] (mnId == 0), erasable[j]
 * (!mbNotErase), th_depth[j] (mThDepth), and the slots slot_off[j] .. slot_off[j + 1]:
 * slot_point (-1: null), slot_level (mvKeysSemantic[i].octave), slot_depth
 * (mvDepth[i]).  The depth rule of :750-751 is evaluated as written: a NaN depth and
 * a depth equal to th_depth are counted; monocular != 0 switches it off.
 * Out: n_mps[j] (nMPs), n_redundant[j] (nRedundantObservations), decision[j]
 * (SIVO_KFCULL_*; 1 and 2 where nRedundantObservations > 0.9 * nMPs in double), and
 * bad_after[p] for every point of the table.  n_mps[j] and n_redundant[j] of a
 * keyframe with decision 3 are left as the caller had them. */
int sivo_keyframe_culling(const SivoObsTable *t, int n_local, const int32_t *local_kf, const uint8_t *is_id0,
                          const uint8_t *erasable, const float *th_depth, const int64_t *slot_off,
                          const int32_t *slot_point, const uint8_t *slot_level, const float *slot_depth, int monocular,
                          int32_t *n_mps, int32_t *n_redundant, uint8_t *decision, uint8_t *bad_after);

enum {
    SIVO_MPCULL_STAYS = 0,         /* LocalMapping.cc:192-194 */
    SIVO_MPCULL_ALREADY_BAD = 1,   /* :181-182 */
    SIVO_MPCULL_FOUND_RATIO = 2,   /* :183-185, SetBadFlag */
    SIVO_MPCULL_OBSERVATIONS = 3,  /* :186-189, SetBadFlag */
    SIVO_MPCULL_AGED_OUT = 4       /* :190-191 */
};

/* The branch of LocalMapping::MapPointCulling (LocalMapping.cc:181-194) each of the n
 * recently added points takes, one thread per point: found = mnFound, visible =
 * mnVisible (the ratio is (float)found / visible < 0.25f in float, MapPoint.cc:281),
 * first_kf_id = mnFirstKFid, n_obs = Observations(), bad = isBad(); current_kf_id =
 * mpCurrentKeyFrame->mnId (both ids are cast to int before the subtraction, :186);
 * the threshold on n_obs is 2 when monocular, else 3.  status[i] = SIVO_MPCULL_*. */
int sivo_mappoint_culling(int n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id,
                          const int32_t *n_obs, const uint8_t *bad, int64_t current_kf_id, int monocular, uint8_t *status);

/* ===========================================================================
 * The tracking thread's local map: Tracking::UpdateLocalMap (reference
 * src/orbslam/Tracking.cc:1087-1235) — the vote, mvpLocalKeyFrames, mpReferenceKF
 * and mvpLocalMapPoints — on a map that stays resident on the device between the
 * frames.  Integer work, exact, the reference's order everywhere.  DESIGN 3.6i.
 * ======================================================================== */
typedef struct sivo_localmap *sivo_localmap_t;

typedef struct {
    int32_t n_kf;              /* keyframes and points are dense indices chosen by the caller */
    int32_t n_points;
    const int64_t *obs_off;    /* n_points + 1, CSR over mObservations (as in SivoObsTable) */
    const int32_t *obs_kf;
    const uint8_t *point_bad;  /* n_points: MapPoint::isBad() */
    const uint8_t *kf_bad;     /* n_kf: KeyFrame::isBad() */
    const int64_t *slot_off;   /* n_kf + 1, CSR over GetMapPointMatches() in slot order */
    const int32_t *slot_point; /* -1 for a null slot */
    const int64_t *covis_off;  /* n_kf + 1, CSR over mvpOrderedConnectedKeyFrames in its order, bad keyframes included; */
    const int32_t *covis_kf;   /* only the first 10 of a list are read (GetBestCovisibilityKeyFrames(10), KeyFrame.cc:222-230) */
    const int64_t *child_off;  /* n_kf + 1, CSR over mspChildren in the order the std::set iterates */
    const int32_t *child_kf;
    const int32_t *parent;     /* n_kf: mpParent, -1 for none */
    const int32_t *kf_order;   /* n_kf, a permutation: the order in which std::map<KeyFrame *, int> walks the keyframes
                                  (Tracking.cc:1156: by pointer value); NULL = 0, 1, 2 ... */
} SivoLocalMapTables;

/* The tables go to the device once and stay there.  For create, replace, set_bad and
 * update: an offset array that does not start at 0 or that decreases, an index outside
 * its range, a kf_order that is not a permutation, a negative count or a NULL array
 * with a non-zero count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched.
 * A handle serves one call at a time (calls from several threads are serialised). */
int sivo_localmap_create(const SivoLocalMapTables *t, sivo_localmap_t *map);
/* A new set of tables into the same handle; its device buffers are reused when they
 * are large enough. */
int sivo_localmap_replace(sivo_localmap_t map, const SivoLocalMapTables *t);
/* point_bad[point_idx[i]] = point_val[i] and kf_bad[kf_idx[i]] = kf_val[i]: all the
 * other threads change between two rebuilds of the map that the update reads.  Of an
 * index listed twice the later entry holds. */
int sivo_localmap_set_bad(sivo_localmap_t map, int n_points, const int32_t *point_idx, const uint8_t *point_val, int n_kf,
                          const int32_t *kf_idx, const uint8_t *kf_val);
int sivo_localmap_destroy(sivo_localmap_t map);

/* What changed in the map since the handle's tables were sent: whole rows, replaced or
 * appended.  Existing indices keep their meaning and nothing is deleted (a removed
 * object stays as a bad row until the next replace); the indices old n_points ..
 * n_points - 1 and old n_kf .. n_kf - 1 are new and every one of them is listed. */
typedef struct {
    uint32_t size;                  /* sizeof(SivoLocalMapDelta) of the caller's header */
    int32_t  n_kf, n_points;        /* the map's sizes AFTER the call; each >= the handle's */
    /* points whose observation list or flag is replaced, appended points included */
    int32_t  n_point_rows;
    const int32_t *point_idx;       /* strictly increasing */
    const int64_t *point_obs_off;   /* n_point_rows + 1, starts at 0 */
    const int32_t *point_obs_kf;    /* in the order std::map<KeyFrame*, size_t> walks */
    const uint8_t *point_bad;       /* n_point_rows */
    /* keyframes whose rows are replaced, appended keyframes included: all rows of a listed keyframe */
    int32_t  n_kf_rows;
    const int32_t *kf_idx;          /* strictly increasing */
    const uint8_t *kf_bad;          /* n_kf_rows */
    const int32_t *kf_parent;       /* n_kf_rows, -1 none */
    const int64_t *kf_slot_off;  const int32_t *kf_slot_point;   /* -1 null slot */
    const int64_t *kf_covis_off; const int32_t *kf_covis_kf;
    const int64_t *kf_child_off; const int32_t *kf_child_kf;
    const int32_t *kf_order;        /* n_kf (new), a permutation; NULL = the handle's order with the
                                       appended keyframes behind it in index order */
} SivoLocalMapDelta;

/* The delta's rows go to the device in one upload and the device builds the new tables
 * from the old ones; one synchronisation.  Afterwards the handle behaves in
 * every call exactly as one created from the full new tables.  A delta with nothing in
 * it (no rows, the handle's sizes, kf_order NULL) does not touch the device.  Refused
 * with SIVO_ERR_INVALID_ARGUMENT before any device is touched, the handle left as it
 * was: a size that is not sizeof(SivoLocalMapDelta), n_kf or n_points below the
 * handle's, point_idx / kf_idx not strictly increasing or out of range, a new index that
 * is not listed, an offset array that does not start at 0 or decreases, a payload index
 * outside the NEW ranges, a kf_order that is not a permutation of the new n_kf, a NULL
 * array with a non-zero count.  An update on another thread sees the old map or the
 * new one. */
int sivo_localmap_apply(sivo_localmap_t map, const SivoLocalMapDelta *delta);
/* out = n_kf, n_points, and the entries of obs_kf, slot_point, covis_kf, child_kf. */
int sivo_localmap_sizes(sivo_localmap_t map, int64_t out[6]);
/* The handle's tables into the caller's writable arrays, sized by sivo_localmap_sizes
 * (an offset array has one entry more than its rows, and is not written where there
 * are no rows); out->n_kf and out->n_points must be the handle's.  kf_order comes back
 * as stored: the identity where the creator passed NULL. */
int sivo_localmap_export(sivo_localmap_t map, SivoLocalMapTables *out);

/* Tracking::UpdateLocalMap (Tracking.cc:1092-1093: UpdateLocalKeyFrames :1126-1235,
 * then UpdateLocalPoints :1096-1124) for one frame: one upload, the launches, one
 * download, one synchronisation.
 * In: frame_point (n_slots = numSemanticKeys) = mCurrentFrame.mvpMapPoints as point
 * indices, -1 for null; kf_premarked / point_premarked = the keyframes / points whose
 * mnTrackReferenceForFrame already equals the frame's id (either may be NULL with a
 * count of 0); prev_local_kf = the mvpLocalKeyFrames the caller holds.
 * Out: *voted = 0 where keyframeCounter is empty (:1144): then local_kf and
 * *n_local_kf are not written, *ref_kf = -1 and the points are those of prev_local_kf,
 * as UpdateLocalPoints still runs.  slot_cleared[i] = 1 where the reference sets
 * mvpMapPoints[i] = nullptr (:1138-1140), else 0.  local_kf[0 .. *n_local_kf) =
 * mvpLocalKeyFrames: every voted keyframe that is not bad in kf_order (:1156-1172, not
 * capped), then for each of those, while the list holds no more than 80 (:1183), the
 * first of its first ten covisibles and the first of its children that are neither bad
 * nor marked, and its parent if not marked (isBad() not tested) — after the first
 * parent the loop ends (:1222-1228).  *ref_kf = pKFmax, the first strict maximum in
 * kf_order among the voted keyframes that are not bad; -1 leaves mpReferenceKF alone.
 * local_point[0 .. *n_local_points) = mvpLocalMapPoints: over the local keyframes in
 * order and their slots in order, the first occurrence of every point that is neither
 * premarked nor bad.  counts (n_kf, may be NULL) = keyframeCounter, 0 where absent.
 * Entries past the counts returned are left as the caller had them.  A list longer than
 * kf_capacity / point_capacity -> SIVO_ERR_CAPACITY and no output is written.
 * The result depends on the handle's tables and this call's arguments alone. */
int sivo_localmap_update(sivo_localmap_t map, int n_slots, const int32_t *frame_point, int n_kf_premarked,
                         const int32_t *kf_premarked, int n_point_premarked, const int32_t *point_premarked, int n_prev,
                         const int32_t *prev_local_kf, int32_t *voted, uint8_t *slot_cleared, int kf_capacity,
                         int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, int point_capacity, int32_t *local_point,
                         int32_t *n_local_points, int32_t *counts);

/* The map points' attributes, resident beside the tables (reference src/orbslam/Tracking.cc:1033-1124:
 * what the second loop of Tracking::SearchLocalPoints and the search behind it read of every
 * local map point).  DESIGN 3.6n.  Per point of the handle: pos = mWorldPos and normal =
 * mNormalVector (3 floats each), min_dist / max_dist = mfMinDistance / mfMaxDistance raw, as
 * sivo_frustum_cull takes them, desc = GetDescriptor() (32 bytes), n_obs = Observations().
 * set_points sends n_rows rows in one upload and scatters them on the device; point_idx is
 * strictly increasing; it may be called any number of times, the later row holds.  A row is
 * SET once a set_points has named it.  sivo_localmap_create starts with every row unset;
 * sivo_localmap_apply keeps every stored row (the store grows by a device copy) and leaves
 * the appended points unset; sivo_localmap_replace unsets all rows, because the caller may
 * have renumbered.  get_points reads rows back (for tests and an adapter's checks):
 * is_set[i] = 1 for a set row; an unset row reads as zeros.
 * A null handle, a negative count, a NULL array with a non-zero count, an index out of range
 * or indices that are not strictly increasing -> SIVO_ERR_INVALID_ARGUMENT before any device
 * is touched, the handle left as it was. */
int sivo_localmap_set_points(sivo_localmap_t map, int n_rows, const int32_t *point_idx, const float *pos, const float *normal,
                             const float *min_dist, const float *max_dist, const uint8_t *desc, const int32_t *n_obs);
int sivo_localmap_get_points(sivo_localmap_t map, int n_rows, const int32_t *point_idx, float *pos, float *normal, float *min_dist,
                             float *max_dist, uint8_t *desc, int32_t *n_obs, uint8_t *is_set);

/* Tracking::UpdateLocalMap and Tracking::SearchLocalPoints in one call (reference
 * src/orbslam/Tracking.cc:1033-1124): sivo_localmap_update with the same arguments, followed by
 * sivo_search_local_points on F over local_point[0 .. *n_local_points) with
 *   pos, normal, min_dist, max_dist, mp_desc, mp_obs [i] = the stored attributes of local_point[i];
 *   skip[i] = 1 where local_point[i] is a frame_point[s] >= 0 with slot_cleared[s] == 0 (the
 *     frame's own points, which the first loop of :1035-1049 stamps) or is listed in seen_point
 *     (the points whose mnLastFrameSeen already equals the frame's id, such as the outliers
 *     dropped at :626-630; may be NULL with n_seen 0); bad points never reach local_point;
 *   occ_obs[k] = n_obs[frame_point[k]] where frame_point[k] >= 0 and the slot is not cleared,
 *     else -1.
 * The update's outputs are sivo_localmap_update's; status, proj_x .. level (per local point;
 * status is required, the others may each be NULL and are written for the points in view only)
 * and *n_to_match, *n_matches are sivo_search_local_points'; match[k] (n_slots) = the position
 * in local_point of the point matched to keypoint k, or -1.  Every output is byte for byte
 * that of the composed pair.  With no local point or nothing in view *n_matches = 0, as the
 * reference skips the search (:1072).  local_point is not sent up again and no per-point
 * host array is built: a kernel reads local_point[i] and the store on the device and writes
 * the search engine's queries, descriptors and blocked flags there.
 * SIVO_ERR_CAPACITY as in sivo_localmap_update; nothing of the search is written then.
 * Beyond sivo_localmap_update's refusals, with SIVO_ERR_INVALID_ARGUMENT before any device is
 * touched: the map and the frame on different devices, n_slots != the frame's keypoint count,
 * frustum->nlevels outside 1 .. 16 or above the frame's, log_scale_factor <= 0, a point row
 * of the handle that is unset (the text names their count and the first index), seen_point
 * out of range. */
int sivo_localmap_search_local_points(sivo_localmap_t map, sivo_mframe_t F, const SivoFrustum *frustum, int n_slots,
                                      const int32_t *frame_point, int n_kf_premarked, const int32_t *kf_premarked,
                                      int n_point_premarked, const int32_t *point_premarked, int n_prev,
                                      const int32_t *prev_local_kf, int n_seen, const int32_t *seen_point, float th, float nn_ratio,
                                      int32_t *voted, uint8_t *slot_cleared, int kf_capacity, int32_t *local_kf, int32_t *n_local_kf,
                                      int32_t *ref_kf, int point_capacity, int32_t *local_point, int32_t *n_local_points,
                                      int32_t *counts, uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos,
                                      int32_t *level, int32_t *match, int *n_to_match, int *n_matches);

#define SIVO_BAWIN_SLOT_NONE (-1)      /* no slot of the keyframe holds the point (a stale observation) */
#define SIVO_BAWIN_SLOT_AMBIGUOUS (-2) /* more than one slot does */

/* The window of Optimizer::LocalBundleAdjustment (reference src/orbslam/Optimizer.cc:496-559,
 * the vertices of :585-622 and the edges of :651-670) on the resident map.  DESIGN 3.6m.
 * In: cand_kf[0] = pKF, cand_kf[1 ..] = pKF->GetVectorCovisibleKeyFrames() in its order
 * (the handle's covis_kf, cut at ten, is not read); kf_local_pre / kf_fixed_pre / point_pre
 * = the keyframes whose mnBALocalForKF / mnBAFixedForKF and the points whose mnBALocalForKF
 * already equal pKF->mnId (each may be NULL with a count of 0).
 * Out: local_kf = the candidates that are not bad, in order; cand_kf[0] is listed whatever
 * its flag (:499).  local_point = over local_kf in order and their slots in order, the first
 * occurrence of every point that is not null, not bad and not in point_pre (:516-533).
 * fixed_kf = over local_point in order and their observation rows in order, the first
 * occurrence of every keyframe that is neither a candidate nor in kf_local_pre nor in
 * kf_fixed_pre, kept where it is not bad (:537-559).  Pose index j is local_kf[j] for
 * j < n_local_kf and fixed_kf[j - n_local_kf] behind that.  For local point i the entries
 * edge_off[i] .. edge_off[i + 1] are its observations in row order whose keyframe is not
 * bad and has a pose index (:670): edge_pose = that index, edge_slot = the one slot s of
 * the keyframe with slot_point[slot_off[k] + s] == p, or SIVO_BAWIN_SLOT_NONE /
 * SIVO_BAWIN_SLOT_AMBIGUOUS (the handle does not store mObservations' idx: the caller
 * resolves those two from its own map).  local_kf and fixed_kf hold kf_capacity entries
 * each, local_point point_capacity, edge_off point_capacity + 1, edge_pose and edge_slot
 * edge_capacity.  counts = n_local_kf, n_local_points, n_fixed_kf, n_edges: written on
 * success and on SIVO_ERR_CAPACITY, where nothing else is written; entries past the counts
 * are left as the caller had them.
 * A null handle, n_cand < 1, an index out of range, a keyframe listed twice in cand_kf (the
 * reference would add its vertex twice), a negative count or a NULL array with a non-zero
 * count -> SIVO_ERR_INVALID_ARGUMENT before any device is touched.  The result depends on
 * the handle's tables and this call's arguments alone. */
int sivo_localmap_ba_window(sivo_localmap_t map, int n_cand, const int32_t *cand_kf, int n_kf_local_pre,
                            const int32_t *kf_local_pre, int n_kf_fixed_pre, const int32_t *kf_fixed_pre, int n_point_pre,
                            const int32_t *point_pre, int kf_capacity, int32_t *local_kf, int32_t *fixed_kf,
                            int point_capacity, int32_t *local_point, int64_t *edge_off, int64_t edge_capacity,
                            int32_t *edge_pose, int32_t *edge_slot, int64_t counts[4]);

/* ===========================================================================
 * Place recognition: the bag-of-words vocabulary and the keyframe database —
 * DBoW2 as ORB-SLAM2 uses it (reference dependencies/DBoW2/DBoW2/TemplatedVocabulary.h,
 * src/orbslam/KeyFrameDatabase.cc:72-322).  Only L1_NORM scoring with TF_IDF
 * weighting (what ORBvoc.txt carries).  DESIGN 3.6f.
 * ======================================================================== */
typedef struct sivo_voc *sivo_voc_t;
typedef struct sivo_bowdb *sivo_bowdb_t;

/* The text format of TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424): a header line
 * `k L scoring weighting`, then one line `parent isLeaf b0 .. b31 weight` per node; node ids in file order from 1,
 * the root is 0; word ids in file order over the leaf lines (:1408-1415).  k <= 20, L <= 10 (:1359); a header other
 * than `k L 0 0` -> SIVO_ERR_INVALID_ARGUMENT with a text that says so.  Beyond the reference: empty lines are
 * skipped, and a parent id that is not an earlier inner node, a parent with more than k children, a truncated line,
 * an inner node without children or an empty file -> SIVO_ERR_INVALID_ARGUMENT.  No device is needed. */
int sivo_voc_create_from_text(const char *path, sivo_voc_t *voc);
/* The same from arrays: entry i describes node i + 1; n_nodes entries (the root is not one of them). */
int sivo_voc_create(int k, int L, int64_t n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                    const double *weight, sivo_voc_t *voc);
/* n_nodes: the root included (m_nodes.size()); n_words: size(). */
int sivo_voc_info(sivo_voc_t voc, int32_t *k, int32_t *L, int64_t *n_nodes, int64_t *n_words);
int sivo_voc_destroy(sivo_voc_t voc);

/* transform(features, BowVector &, FeatureVector &, levelsup) (TemplatedVocabulary.h:1126-1194) with the descent of
 * :1217-1259 for n descriptors of 32 bytes.  Per feature: word[i], and node[i] = the node at level L - levelsup (0 when
 * levelsup >= L; the leaf's own id when the descent ends above that level, where the reference leaves it
 * uninitialised).  The BowVector: *n_words pairs (bow_words ascending, bow_values); the FeatureVector in CSR form:
 * *n_fv_nodes node ids ascending, fv_offsets (*n_fv_nodes + 1 entries), fv_features ascending within a node.  A word of
 * weight 0 is in neither.  Values bit-identical to the reference's order of operations.  Every array holds n entries
 * (fv_offsets n + 1).  n > SIVO_BOW_SET_CAP or levelsup < 0 -> SIVO_ERR_INVALID_ARGUMENT. */
#define SIVO_BOW_SET_CAP 8192
int sivo_bow_transform(sivo_voc_t voc, const uint8_t *desc, int n, int levelsup, int32_t *word, int32_t *node,
                       int32_t *bow_words, double *bow_values, int32_t *n_words, int32_t *fv_nodes, int32_t *fv_offsets,
                       int32_t *fv_features, int32_t *n_fv_nodes);
/* Several sets in one call: set s owns the descriptors offsets[s] .. offsets[s + 1] and the same range of every array;
 * its fv_offsets start at offsets[s] + s; n_words / n_fv_nodes have n_sets entries.  Equal to the single calls. */
int sivo_bow_transform_batch(sivo_voc_t voc, const uint8_t *desc, const int64_t *offsets, int n_sets, int levelsup,
                             int32_t *word, int32_t *node, int32_t *bow_words, double *bow_values, int32_t *n_words,
                             int32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features, int32_t *n_fv_nodes);
/* KeyFrameDatabase's stored BowVectors, resident on the device.  add: n (word ascending, value) pairs -> *slot (slots
 * count up from 0).  erase leaves a tombstone.  clear forgets every slot (the next add is slot 0). */
int sivo_bowdb_create(sivo_voc_t voc, sivo_bowdb_t *db);
int sivo_bowdb_add(sivo_bowdb_t db, const int32_t *words, const double *values, int n, int32_t *slot);
int sivo_bowdb_erase(sivo_bowdb_t db, int32_t slot);
int sivo_bowdb_clear(sivo_bowdb_t db);
int sivo_bowdb_destroy(sivo_bowdb_t db);
int sivo_bowdb_size(sivo_bowdb_t db, int32_t *n_slots);
/* One launch over every slot.  Per slot: common = the number of words shared with the query (mnLoopWords /
 * mnRelocWords, KeyFrameDatabase.cc:82-102, :211-229; 0 for a tombstone), first_word = the smallest shared word id or
 * -1, score = L1Scoring::score (ScoringObject.cpp:23-68): the terms |v - w| - |v| - |w| of the shared words added in
 * ascending word order, then -sum / 2.  The arrays hold *n_slots = sivo_bowdb_size entries. */
int sivo_bowdb_query(sivo_bowdb_t db, const int32_t *q_words, const double *q_values, int nq, int32_t *common,
                     int32_t *first_word, double *score, int32_t *n_slots);

/* ===========================================================================
 * The two map corrections of the loop closer: LoopClosing::CorrectLoop's pose
 * propagation and point correction (reference src/orbslam/LoopClosing.cc:436-526)
 * and the map update behind the global bundle adjustment (LoopClosing.cc:694-753).
 * Sim3 arithmetic in double in Eigen's operation order, cv::Mat arithmetic in float
 * under OpenCV's gemm rules, the reference's sequential effects reproduced: equal to
 * the reference's loops bit for bit.  Every NaN leaves as 0x7FC00000 (float) or
 * 0x7FF8000000000000 (double).  DESIGN 3.6j.
 * For both calls: a negative count, a NULL array with a non-zero count, an offset
 * array that does not start at 0 or that decreases, an index outside its table, or
 * one of the conditions named below -> SIVO_ERR_INVALID_ARGUMENT with a message of
 * its own, before any device is touched.
 * ======================================================================== */
typedef struct {
    int32_t n_kf;              /* >= 1: the keyframes of CorrectedSim3 in the order that std::map iterates (by pointer) */
    int32_t cur;               /* index of mpCurrentKF among them */
    int32_t n_all;             /* >= n_kf: the keyframe table; entries n_kf .. are observers / reference keyframes only */
    int32_t n_points;
    const float *tiw;          /* 16 n_kf: GetPose(), row-major */
    const float *twc_cur;      /* 16: mpCurrentKF->GetPoseInverse() */
    const double *scw;         /* 8: mg2oScw as qx qy qz qw tx ty tz s; s > 0 */
    const float *ow;           /* 3 n_all: GetCameraCenter() */
    const int64_t *slot_off;   /* n_kf + 1, CSR over GetMapPointMatches() of each corrected keyframe */
    const int32_t *slot_point; /* a point index, -1 for a null slot */
    const float *pos;          /* 3 n_points: GetWorldPos() */
    const uint8_t *skip;       /* n_points: isBad() || mnCorrectedByKF == mpCurrentKF->mnId on entry */
    const int64_t *obs_off;    /* n_points + 1, CSR over mObservations in its order, all observations (as sivo_mappoint_refresh) */
    const int32_t *obs_kf;     /* indices into the keyframe table */
    const int32_t *ref_kf;     /* n_points: mpRefKF in the table; -1 only for a point that no slot would move */
    const float *level_scale;  /* n_points, as sivo_mappoint_refresh */
    const float *last_scale;
    double *noncorrected_siw;  /* out, 8 n_kf: NonCorrectedSim3 */
    double *corrected_siw;     /* out, 8 n_kf: CorrectedSim3 */
    float *tiw_out;            /* out, 16 n_kf: the pose SetPose receives, [R t/s; 0 0 0 1] */
    float *ow_out;             /* out, 3 n_kf: the camera centre after that SetPose */
    int32_t *corrected_by;     /* out, n_points: the keyframe that moved the point (mnCorrectedReference), -1: untouched */
    float *pos_out;            /* out, 3 n_points     } written for the moved points only; normal and the distances */
    float *normal;             /* out, 3 n_points     } only where flags comes back 0 */
    float *max_dist;           /* out, n_points       } */
    float *min_dist;           /* out, n_points       } */
    uint8_t *flags;            /* out, n_points: 0 or SIVO_MP_NO_OBSERVATION } */
} SivoLoopCorrect;

/* LoopClosing.cc:447-526 on arrays.  Keyframe i: NonCorrected = Sim3(Quaterniond(Riw), tiw, 1), the quaternion not
 * normalised; Corrected = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc one float gemm, scw verbatim for i == cur; the
 * new pose is [toRotationMatrix(q) t * (1 / s)] narrowed to float, its camera centre KeyFrame::SetPose's.  A point is
 * moved by the first keyframe of the given order that holds it in a slot, once: pos_out = (float)
 * CorrectedSwi.map(Siw.map((double)pos)).  UpdateNormalAndDepth runs at that moment: keyframe i's SetPose follows its
 * point loop, so for a point moved by keyframe i the camera centre of keyframe k is ow_out[k] where k < n_kf and
 * k < i, else ow[k].  Also refused: cur outside [0, n_kf), scw[7] <= 0 or NaN, ref_kf < 0 for a point that would be
 * moved. */
int sivo_loop_correct(const SivoLoopCorrect *problem);

enum {
    SIVO_GBA_POINT_BAD = 0,         /* LoopClosing.cc:726 */
    SIVO_GBA_POINT_FROM_BA = 1,     /* :729-731, pos_out = pos_gba */
    SIVO_GBA_POINT_CARRIED = 2,     /* :733-751, through the reference keyframe's pose before and after */
    SIVO_GBA_POINT_REF_OUTSIDE = 3  /* :737, untouched */
};

typedef struct {
    int32_t n_kf;
    int32_t n_origins;
    int32_t n_points;
    const int32_t *origin;     /* n_origins: mvpKeyFrameOrigins */
    const int64_t *child_off;  /* n_kf + 1, CSR over GetChildren() (as in SivoLocalMapTables) */
    const int32_t *child_kf;
    const float *tcw;          /* 16 n_kf: GetPose(); GetPoseInverse() is derived from it by KeyFrame::SetPose's rules */
    float *tcw_gba;            /* in/out, 16 n_kf: mTcwGBA */
    uint8_t *in_gba;           /* in/out, n_kf: mnBAGlobalForKF == nLoopKF */
    float *tcw_bef;            /* in/out, 16 n_kf: mTcwBefGBA */
    const float *pos;          /* 3 n_points: GetWorldPos() */
    const float *pos_gba;      /* 3 n_points: mPosGBA */
    const uint8_t *point_in_gba; /* n_points: mnBAGlobalForKF == nLoopKF */
    const uint8_t *point_bad;  /* n_points: isBad() */
    const int32_t *ref_kf;     /* n_points: GetReferenceKeyFrame(); -1 only for a bad point or one the BA holds */
    float *tcw_out;            /* out, 16 n_kf: the pose SetPose receives; written for the reached keyframes only */
    float *ow_out;             /* out, 3 n_kf: its camera centre; likewise */
    uint8_t *kf_reached;       /* out, n_kf: the walk from the origins came by */
    float *pos_out;            /* out, 3 n_points: written for SIVO_GBA_POINT_FROM_BA and SIVO_GBA_POINT_CARRIED only */
    uint8_t *point_status;     /* out, n_points: SIVO_GBA_POINT_* */
} SivoGbaPropagate;

/* LoopClosing.cc:695-753 on arrays.  The walk from the origins through the children: a reached keyframe outside the BA
 * gets tcw_gba = (tcw_child * Twc_parent) * tcw_gba_parent — two float gemms on the parent's pose and inverse from
 * before its SetPose — and in_gba = 1; every reached keyframe gets tcw_bef = tcw and tcw_out = tcw_gba (an origin
 * outside the BA with its stale tcw_gba, as the reference); unreached keyframes keep everything.  The points read
 * in_gba after the walk: Xc = Rcw_bef * P + tcw_bef, pos_out = Rwc * Xc + twc with the reference keyframe's new inverse
 * pose, each one gemm.  Also refused: a keyframe listed as a child more than once, an origin that is somebody's child
 * or is listed twice, a cycle among the children (the kernels walk the tree), ref_kf < 0 for a point that would be
 * carried. */
int sivo_gba_propagate(const SivoGbaPropagate *problem);

#ifdef __cplusplus
}
#endif
#endif /* SIVO_HIP_H */
