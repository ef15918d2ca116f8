/*
 * expecto_hip.h -- C-ABI of the MI355X-native ExPecto Beluga hot path (gfx950).
 *
 * Every entry point takes plain pointers and sizes; device pointers are HIP device
 * memory, `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 * functions return 0 on success and a negative status on failure; the message of the
 * last failure on the calling thread is returned by expecto_last_error().
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *   expecto_beluga_create          Beluga() + load_state_dict(torch.load(pth)) + .cuda()
 *                                  (Beluga.py:18-48; chromatin.py:102-106;
 *                                   compute_expecto_features.py:36-40)
 *   expecto_beluga_forward_onehot  Beluga.forward(x[B,4,1,2000]) -> [B,2002]
 *                                  (Beluga.py:50-51; called at chromatin.py:270,278,
 *                                   compute_expecto_features.py:121-122)
 *   expecto_beluga_forward_codes   encodeSeqs(...) one-hot + Beluga.forward, fused: the
 *                                  one-hot / reverse-complement of chromatin.py:153-171
 *                                  is generated from base codes inside the conv1 + conv2
 *                                  k-mer gather (or the conv1 kernel)
 *   expecto_variant_windows        fetchSeqs window splice for SNVs (chromatin.py:175-209)
 *                                  from a device-resident genome
 *   expecto_indel_windows          fetchSeqs splice + centre crop for indels / MNPs
 *                                  (chromatin.py:164,202-209) from a device-resident genome
 *   expecto_tss_windows            TSS tiling genome.sequence(...) + encodeSeqs
 *                                  (compute_expecto_features.py:107-113)
 *   expecto_diff                   diff = alt - ref (chromatin.py:281)
 *   expecto_fwd_rc_average         (x[:N] + x[N:]) / 2 (predict.py:186-190;
 *                                   0.5*(fwd+rc) of compute_expecto_features.py:123)
 *   expecto_tss_reduce             pos_weights x pred_fwd_rc (compute_expecto_features.py:91-124)
 *   expecto_variant_reduce(_lut)   exp-decay shift weights x effects (predict.py:87-136)
 *   expecto_variant_contrib        per-mark and per-cluster attribution of the expression effect
 *                                  (predict_by_cluster.py:73-109, predict_by_cluster_rsat.py:105-144)
 *   expecto_gblinear_predict       xgboost gblinear scoring of feature rows (predict.py:150-166)
 *   expecto_gblinear_train_round   one xgb.train boosting round of gblinear / reg:linear models
 *                                  (train.py:140-146, train_bootstrap.py:88-106)
 *   expecto_gblinear_train_round_hp  the same round with eta / lambda / alpha / lambda_bias per model
 *   expecto_gblinear_predict_cols  bst.predict(dtrain / dtest) on the training matrix (train.py:147)
 *   expecto_gblinear_rmse          the eval-rmse / train-rmse of xgb.train's evallist (train.py:144-146)
 *   expecto_shift_reduce           200-shift reduction of consensus / eQTL sequences
 *                                  (geuvadis_sed_for_top_eqtls.py:95-121, geuvadis_predict_consensus.py:110-128)
 *   expecto_pairwise_euclidean     scipy's pdist under AgglomerativeClustering().fit
 *   expecto_ward_linkage           and its Ward linkage (interpret_features.py:99-120,
 *                                  interpret_features_grouped.py:103-146)
 *   expecto_square_distances       scipy's squareform of those distances
 *   expecto_silhouette_node_sums   the per-cluster distance sums of silhouette_samples, once per tree node
 *   expecto_silhouette_cuts        silhouette_samples of every cut (interpret_features_grouped.py:120-144)
 *   expecto_tfidf_stats / _gram    tf-idf of the mark tracks and its float64 Gram matrix (svd.py:76-85)
 *   expecto_tfidf_project          components_ of the truncated SVD (svd.py:84-85)
 *   expecto_tfidf_transform        svd.transform(tf_idf) (svd_transform.py:80)
 *   expecto_kmeans_plusplus        the k-means++ seeding and
 *   expecto_kmeans_lloyd           the Lloyd iteration of KMeans(n_clusters=k).fit(X), batched over k and
 *                                  restarts (cluster_and_viz.py:45-58, the elbow sweep among them)
 *   expecto_tsne_affinities        the perplexity search and joint probabilities and
 *   expecto_tsne_descend           the gradient descent of TSNE(n_components=2, method='exact').fit_transform(X)
 *                                  (cluster_and_viz.py:60-66)
 *   expecto_knn_jaccard            the k-nearest-neighbour graph with Jaccard weights and
 *   expecto_louvain                the Louvain communities of it, batched over resolutions and restarts
 *                                  (cluster_and_viz_louvain.py:48-53)
 *   expecto_cluster_enrich        the counting of cluster_contribs_hypergeom, batched over the data, the
 *                                  shuffled controls and the SED quartiles (cluster_analysis_with_fimo.py:126-162)
 *   expecto_hypergeom_sf           its scipy.stats.hypergeom.sf (cluster_analysis_with_fimo.py:163)
 *   expecto_pwm_pvalues            the score-to-p-value tables of `fimo` (query_fimo_for_predictions.py:45) and
 *   expecto_pwm_scan               its matches, reduced to the best one that overlaps the variant per motif
 *                                  and sequence (query_fimo_for_predictions.py:53-57)
 *   expecto_pwm_compare            the pairwise motif comparison (cor, Ncor over all offsets, both strands),
 *   expecto_average_linkage        the tree and
 *   expecto_linkage_threshold_cut  the clusters that follow cluster_by_pwm.py's cluster_motifs.jaspar
 *   expecto_rank2_f32 / _f64       scipy's rankdata inside spearmanr (train.py:150,163; train_bootstrap.py:110,124)
 *   expecto_model_metrics          pearsonr, spearmanr and r2_score of a model's predictions
 *                                  (train_susztak.py:153-154; train.py:163,171-172; train_bootstrap.py:124,132-133;
 *                                   geuvadis_predict_consensus.py:254-256 and its _for_top_eqtls copy)
 *   expecto_bootstrap_coef_stats   np.std(ddof=1) / np.mean over the bootstrap models, the z-score and the
 *                                  coefficient of variation (plot_bootstrapped_coefficients.py:56,64,75)
 *   expecto_ism_variants / _score  no reference script: saturation mutagenesis, i.e. every SNV of a region
 *   expecto_ism_summary            through chromatin.py, make_closest_genes_file.py and predict.py per model
 *   expecto_ecdf_tail_counts       no reference script: e-values of effects against a background variant set,
 *   expecto_ecdf_summary           this project's definitions
 *   expecto_beluga_destroy         (model teardown)
 */
#ifndef EXPECTO_HIP_H
#define EXPECTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct expecto_beluga* expecto_beluga_t;

enum {
  EXPECTO_OK = 0,
  EXPECTO_EINVAL = -1,   /* bad argument (shape, pointer, mode)            */
  EXPECTO_EHIP = -2,     /* HIP runtime error                              */
  EXPECTO_ENOMEM = -3,   /* device allocation failed                       */
};

/* Strand modes of expecto_beluga_forward_codes. */
enum {
  EXPECTO_STRAND_FWD = 0,   /* n output rows: the windows as given                       */
  EXPECTO_STRAND_RC = 1,    /* n output rows: reverse complement of each window          */
  EXPECTO_STRAND_BOTH = 2,  /* 2n output rows: [fwd rows 0..n-1 ; rc rows n..2n-1]
                               (encodeSeqs row order, chromatin.py:170-171)             */
};

/* GEMM arithmetic (expecto_beluga_set_precision).  All accumulate in fp32:
 *  FP32   exact fp32 products and accumulation (v_mfma_f32_32x32x2_f32);
 *  BF16X6 every fp32 operand split exactly into three bf16 terms, the six products of
 *         combined order <= 2 accumulated in fp32 (v_mfma_f32_16x16x32_bf16); representation
 *         error < 2^-24 relative, products exact, over fp32's whole exponent range;
 *  F16X3  operands scaled by powers of 2 (weights per output channel; activations per layer,
 *         calibrated once per handle on a seeded batch) and split into two fp16 terms
 *         (22 significant bits), three products per k (v_mfma_f32_16x16x32_f16) -- half the
 *         MFMA work of BF16X6.  An activation that does not fit fp16 after scaling raises an
 *         overflow flag and the whole call is recomputed with BF16X6 (counted by
 *         expecto_beluga_f16_fallbacks), so F16X3 never returns a saturated result. */
enum {
  EXPECTO_PRECISION_FP32 = 0,
  EXPECTO_PRECISION_BF16X6 = 1,
  EXPECTO_PRECISION_F16X3 = 2,
};

/* Number of parameter tensors and their order (the reference state-dict keys,
 * SURVEY.md 2.2): model.0.{0,2,6,8,12,14}.{weight,bias}, model.1.2.1.{weight,bias},
 * model.1.4.1.{weight,bias}. */
#define EXPECTO_BELUGA_NPARAMS 16
#define EXPECTO_BELUGA_INPUT_LEN 2000
#define EXPECTO_BELUGA_NFEAT 2002

/* Build a model handle on `device`.  `params` are 16 DEVICE pointers to fp32 tensors in
 * the reference layouts (conv weight [Cout,Cin,1,8], fc weight [out,in]); they are
 * repacked into the kernels' layouts, so the caller may free them afterwards.
 * `max_batch` bounds the windows processed per internal chunk (workspace size).
 * The handle also builds (or shares, with other handles of this device holding the same
 * conv1 / conv2 weights) the k-mer tables its forwards from base codes gather conv1 + conv2
 * + pool1 from: 20.7 GB, ~40 ms, freed with the last handle using them; if they do not fit,
 * conv2 runs on the MFMAs.  EXPECTO_CONV2_TABLE=0 skips them. */
int expecto_beluga_create(int device, const float* const* params, int max_batch, void* stream,
                          expecto_beluga_t* out);
void expecto_beluga_destroy(expecto_beluga_t h);

/* Bytes of device memory the handle owns (weights + workspace) plus the k-mer tables it
 * holds (20.7 GB) if it is their first live holder: summed over handles that share one set of
 * tables, the tables count once. */
size_t expecto_beluga_device_bytes(expecto_beluga_t h);

/* 1 if the handle's forwards from base codes (and exact one-hot floats) gather conv1 + conv2 +
 * pool1 from the k-mer tables, 0 if they run conv1 / conv2 on the MFMAs (same parity bar, other
 * bits; about -25 % throughput).  *reason (may be NULL): 0 tables held, 1 switched off
 * (EXPECTO_CONV2_TABLE=0), 2 no room (the device allocation failed, or the tables exceed
 * EXPECTO_KMER_MAX_BYTES; the library then prints one line on stderr at creation). */
int expecto_beluga_conv2_table_active(expecto_beluga_t h, int* reason);

/* F16X3 computes FC1 (Beluga.py:43-44) as a block-Karatsuba convolution over 25-row blocks of the
 * conv6 rows: 4 windows 400 bp apart in one pool2-phase block of a segment share 9 block products
 * instead of 16 (DESIGN.md "FC1 as a block-Karatsuba convolution"; EXPECTO_FC1_KARATSUBA=0: the
 * direct FC1).  A window's FC1 is a sum of products of its own rows fixed by its ROLE, its position
 * in such a group: on the segment path (conv6 offset / 25) mod 4, every per-window forward (codes,
 * one-hot, pairs) the handle's role, 0 by default.  Role 4 is the direct FC1: segment-pair calls in
 * which more than a third of the windows hold the SNV run it for every window (their alt windows
 * would recompute nearly every product).  A window computed in the same role gives the same bits
 * on every path; other roles agree to the parity bar.  Sets the per-window role (0..4). */
int expecto_beluga_set_fc1_role(expecto_beluga_t h, int role);

/* y[n,2002] = Beluga.forward(x[n,4,1,2000]) (x contiguous fp32, any values).  When the handle
 * holds the k-mer tables, runs F16X3 or BF16X6, x is 16-byte aligned and every column of x is an
 * exact one-hot column (one 1.0f, three +0.0f) or all zeros, as encodeSeqs writes them
 * (chromatin.py:138-172), the call converts x to base codes and equals
 * expecto_beluga_forward_codes(FWD) bit for bit; otherwise conv1 / conv2 run on the MFMAs.  The
 * check costs one pass over x and one stream sync. */
int expecto_beluga_forward_onehot(expecto_beluga_t h, const float* x, int n, float* y, void* stream);

/* Windows given as base codes (uint8, 0=A 1=G 2=C 3=T 4=zero column for N/n/H/-),
 * window i at codes + i*code_stride, 2000 codes each.  y has n rows (FWD, RC) or 2n rows
 * (BOTH). */
int expecto_beluga_forward_codes(expecto_beluga_t h, const uint8_t* codes, int n, long long code_stride,
                                 int strand_mode, float* y, void* stream);

/* Windows that are slices of longer sequences ("segments") with a shared trunk: segment i
 * is seg_len codes at codes + i*code_stride (seg_len % 4 == 0); window w is the 2000 codes at
 * offset win_off[w] (a multiple of 4) of segment win_seg[w] (HOST arrays, sorted by segment).
 * conv1..conv4 run once per segment, conv5/conv6 once per (segment, pool2 phase), FC once per
 * window; every output equals the per-window forward bit for bit.  y has n_win rows (FWD:
 * the windows; RC: their reverse complements) or 2*n_win rows (BOTH: fwd rows then rc rows);
 * window w lands in row win_row[w] of its strand block (HOST array, a permutation of
 * 0..n_win-1; NULL = row w).
 * Replaces the per-shift re-encoding + forward of chromatin.py:243-279 and the 200-window
 * TSS tiling of compute_expecto_features.py:105-122. */
int expecto_beluga_forward_segments(expecto_beluga_t h, const uint8_t* codes, int n_seg, int seg_len,
                                    long long code_stride, int strand_mode, const int* win_seg, const int* win_off,
                                    const int* win_row, int n_win, float* y, void* stream);

/* Genome slices for segments: codes[i*seg_len + j] = genome[start[i] + j] (zero code outside
 * [0, genome_len)), with codes[i*seg_len + splice_pos[i]] = splice_code[i] when splice_code
 * is not NULL (the fetchSeqs allele splice of chromatin.py:209 for SNVs). */
int expecto_gather_segments(const uint8_t* genome, long long genome_len, const long long* start, int n,
                            int seg_len, const int* splice_pos, const uint8_t* splice_code, uint8_t* codes,
                            void* stream);

/* SNV ref/alt window pairs with alt-cone reuse: ref_codes/alt_codes are n windows each
 * (2000 codes at + v*code_stride) that differ at most at window index var_pos[v] (DEVICE array).
 * The ref windows run the full forward; each alt window recomputes, layer by layer, only the
 * rows the SNV changes (conv1 8, pool1 5, conv3 12, pool2 6, conv5 13, conv6 20 rows) from
 * input patches assembled out of the ref activations, so the alt trunk costs ~6 % of a window
 * -- outputs are bit-identical to the full alt forward.
 * strand_mode FWD (rows: fwd) or BOTH (fwd and reverse complement).  Output row of (strand s,
 * variant v) is s*strand_stride + v in y_ref and in y_alt (chromatin.py:262-281 row order
 * when strand_stride = n). */
int expecto_beluga_forward_pairs(expecto_beluga_t h, const uint8_t* ref_codes, const uint8_t* alt_codes, int n,
                                 long long code_stride, const int* var_pos, int strand_mode, float* y_ref,
                                 float* y_alt, long long strand_stride, void* stream);

/* SNV shift sweeps on the segment path with alt reuse: segment i (as in
 * expecto_beluga_forward_segments) is the REF sequence; its alt sequence has code
 * alt_code[i] (DEVICE array) at index var_pos[i] (HOST array, 0 <= var_pos[i] < seg_len).
 * Both alleles' windows are computed (same win_* tables): the ref trunk once per segment, and
 * for the alt only the rows the SNV changes at each layer (conv1 8, pool1 5, conv3 12, conv4
 * 19, pool2 6 per phase, conv5 13, conv6 20), assembled from the ref activations; alt windows
 * that do not hold the SNV equal their ref window and get a copy of its row -- bit-identical
 * to the full alt forward.  Window w of strand s lands in row s*strand_stride + win_row[w] of y_ref and of
 * y_alt.  Replaces the ref/alt forwards of chromatin.py:243-281 for --maxshift sweeps (and
 * the 200-shift eQTL variant scoring of geuvadis_sed_for_top_eqtls.py:61-98). */
int expecto_beluga_forward_segment_pairs(expecto_beluga_t h, const uint8_t* codes, const int* var_pos,
                                         const uint8_t* alt_code, int n_seg, int seg_len, long long code_stride,
                                         int strand_mode, const int* win_seg, const int* win_off, const int* win_row,
                                         int n_win, float* y_ref, float* y_alt, long long strand_stride,
                                         void* stream);

/* Select the GEMM arithmetic for later calls (a new handle starts in F16X3).  F16X3's fp16
 * weight planes and activation scales are built at handle creation: a BF16X6 forward of 256
 * seeded random windows; each layer's scale puts its largest calibration activation at
 * 2^target_log2, default 10, leaving >= 2^5 of headroom below fp16's 65504 before the
 * fallback. */
int expecto_beluga_set_precision(expecto_beluga_t h, int precision);
int expecto_beluga_get_precision(expecto_beluga_t h);
/* F16X3 calibration target (log2 of the scaled calibration maximum, 0..20); re-derives the
 * scales.  Tests use a large target to force the overflow fallback. */
int expecto_beluga_set_f16_target(expecto_beluga_t h, int target_log2);
/* F16X3 state: activation scale exponents of the 7 layer inputs (conv2..fc2) into sx[7];
 * returns the number of calls recomputed with BF16X6 after an overflow (or < 0 on error). */
long long expecto_beluga_f16_fallbacks(expecto_beluga_t h, int* sx);

/* F16X3 overflow check mode.  deferred = 0 (default): every forward call reads the device
 * overflow flag when its kernels are done (one stream sync per call) and recomputes itself with
 * BF16X6 if an activation did not fit fp16, so outputs are final when the call returns.
 * deferred = 1: calls only enqueue work (no host sync inside a forward); the flag stays set on
 * the device until expecto_beluga_overflow_pending() is called at the caller's release point
 * (before outputs are copied out), which syncs `stream`, returns 1 if any call since the last
 * check overflowed (and clears the flag; the caller then recomputes those calls with BF16X6),
 * else 0 (< 0 on error).  One exception to "no host sync": expecto_beluga_forward_onehot on a
 * handle that holds the k-mer tables runs a one-hot check pass over x and syncs once per call to
 * pick its path (codes through the tables, or the MFMA conv1 / conv2 for other floats) before it
 * enqueues the forward; EXPECTO_ONEHOT_CODES=0 (always the MFMA path) or forward_codes avoid it. */
int expecto_beluga_set_overflow_check(expecto_beluga_t h, int deferred);
int expecto_beluga_overflow_pending(expecto_beluga_t h, void* stream);
/* Deferred mode, streamed batches: enqueue on `stream` a copy of the flag into *dst (pinned host
 * or device memory) followed by its reset, without a host sync.  Enqueued right after a batch's
 * forward calls, *dst holds exactly that batch's overflow state once an event recorded after it
 * has completed (the stream runs in order), while later batches are already queued. */
int expecto_beluga_overflow_take(expecto_beluga_t h, int* dst, void* stream);
/* Deferred mode: the caller acted on a flag obtained through expecto_beluga_overflow_take and
 * recomputed that batch with BF16X6; adds one to the count expecto_beluga_f16_fallbacks reports
 * (expecto_beluga_overflow_pending counts its own). */
int expecto_beluga_count_fallback(expecto_beluga_t h);

/* Per-layer device time accumulated over forward calls while profiling is on (ms), launches
 * (`calls`) and executed multiply-adds (`macs`: GEMM M x N x K actually run, including the
 * few padding rows; reuse paths execute fewer than the dense per-window count).
 * Layers: 0 conv1, 1 conv2, 2 conv3, 3 conv4 (+ pool2 on the segment/patch paths), 4 conv5,
 * 5 conv6, 6 fc1, 7 fc1-reduce, 8 fc2; entries 9..17 are the same layers' alt-delta launches
 * (forward_pairs / forward_segment_pairs), timed apart from the full-window launches.
 * Fills min(max_layers, 18) entries and returns 18. */
int expecto_beluga_set_profiling(expecto_beluga_t h, int on);
int expecto_beluga_layer_times(expecto_beluga_t h, double* ms, long long* calls, double* macs, int max_layers);

/* While profiling, every conv GEMM launch (conv2-6) is also timed alone -- its own HIP event pair on
 * the launch stream, without the pool2 pass that shares the conv4 slot -- and logged by (slot, rows).
 * Returns the group of slot `slot` (layer_times numbering) with the most rows: the full-size
 * launches, *rows each, *calls of them, their summed *ms and executed *macs.  bench.py's roofline
 * reads this (the rocprofv3 launch_groups.csv of the same command lists the same launches). */
int expecto_beluga_main_launches(expecto_beluga_t h, int slot, long long* rows, double* ms, long long* calls,
                                 double* macs);

/* SNV windows from a device-resident genome (uint8 codes as above).  For variant v and
 * shift s the 2000-code window is genome[off_v + shift - 999 + i], i = 0..1999, with the
 * code at index 999 - shift replaced by ref_code[v] (allele 0) or alt_code[v] (allele 1)
 * (chromatin.py:202-209 then the centre crop of :164).  off_v = 0-based genome offset of
 * the variant base.  Output codes[((a*n_shift + j)*n + v)*2000 + i] for allele a in {0,1}. */
int expecto_variant_windows(const uint8_t* genome, long long genome_len, const long long* var_off,
                            const uint8_t* ref_code, const uint8_t* alt_code, int n,
                            const int* shifts, int n_shift, uint8_t* codes, void* stream);

/* Indel / MNP windows (chromatin.py:202-209, centre crop :164).  Item t's 2100-base fetch
 * window starts at 0-based genome offset start0[t]; the allele (lalt[t] codes at
 * allele_codes[allele_off[t]..]) replaces lref[t] bases at mutpos[t]; output
 * codes[t*2000 + i] = S[crop[t] + i] of the spliced sequence S (crop = floor((len(S)-2000)/2)).
 * Callers keep items with a window past the contig, mutpos < 0, mutpos + lref > 2100 or
 * len(S) < 2000 on the host (the reference's Python-slicing corner cases). */
int expecto_indel_windows(const uint8_t* genome, long long genome_len, const long long* start0,
                          const int* mutpos, const int* lref, const int* lalt, const int* crop,
                          const int* allele_off, const uint8_t* allele_codes, int n, uint8_t* codes,
                          void* stream);

/* TSS tiling windows (compute_expecto_features.py:107-111): gene g, shift j covers the
 * 0-based genome offsets tss_off[g] + shifts[j]*strand[g] - 999 + i, i = 0..1999
 * (strand = +1/-1).  Output codes[(g*n_shift + j)*2000 + i]. */
int expecto_tss_windows(const uint8_t* genome, long long genome_len, const long long* tss_off, const int8_t* strand,
                        int n_genes, const int* shifts, int n_shift, uint8_t* codes, void* stream);

/* out[i] = a[i] - b[i], i < count (fp32). */
int expecto_diff(const float* alt, const float* ref, long long count, float* out, void* stream);

/* out[r, f] = (x[r, f] + x[r + rows, f]) / 2 for r < rows, f < cols (fp32). */
int expecto_fwd_rc_average(const float* x, int rows, int cols, float* out, void* stream);

/* TSS reduction for n_genes genes: fwd and rc are [n_genes, n_shift, nfeat] fp32;
 * weights [10, n_shift] fp64; out [n_genes, 10*nfeat] fp64 with
 * out[g, k*nfeat + f] = sum_s weights[k,s] * (0.5f*(fwd[g,s,f] + rc[g,s,f])).
 * The reductions below stage their weights in 64 KiB of LDS: n_shift <= 819 (EXPECTO_EINVAL
 * otherwise; the reference sweeps 9 to 201 shifts). */
int expecto_tss_reduce(const float* fwd, const float* rc, const double* weights, int n_genes, int n_shift,
                       int nfeat, double* out, void* stream);

/* Variant reduction: effects [n_shift, n, nfeat] fp32 (fwd/rc-averaged, shift order of
 * chromatin.py:243), dist[n] (pos - TSS, int64), strand_plus[n] (1 '+', 0 '-'),
 * shifts[n_shift]; out [n, 10*nfeat] fp64 (predict.py:87-124 feature layout). */
int expecto_variant_reduce(const float* effects, const long long* dist, const uint8_t* strand_plus,
                           const int* shifts, int n_shift, int n, int nfeat, double* out, void* stream);
/* The same with the decay factors from a table: exp_lut[k*lut_len + fl] = exp(-c_k * fl)
 * (c = 0.01, 0.02, 0.05, 0.1, 0.2; DEVICE array) computed by the caller with the reference's
 * own exp (numpy, predict.py:88-107), so the features equal the reference's bit for bit;
 * expecto_variant_reduce uses the device exp (within 1 ulp).  A distance whose fl =
 * floor(|d|/200) is >= lut_len takes the device exp too (never a read past the table). */
int expecto_variant_reduce_lut(const float* effects, const long long* dist, const uint8_t* strand_plus,
                               const int* shifts, int n_shift, int n, int nfeat, const double* exp_lut, int lut_len,
                               double* out, void* stream);

/* Attribution of the expression effect to chromatin marks and mark clusters
 * (predict_by_cluster.py:73-109, predict_by_cluster_rsat.py:105-144), fused with the variant
 * reduction so that the [n, 10*nfeat] feature matrices never exist.  Every pointer is a DEVICE
 * pointer.  eff_ref, eff_alt, dist, strand_plus, shifts, exp_lut, lut_len: as
 * expecto_variant_reduce_lut (same n_shift and n limits).  keep[nk]: the kept mark columns,
 * ascending, each in 0..nfeat-1.  w[n_models, 10*nk] f64: the weights as the reference parses
 * them from the text dump, index k*nk + f.  Clusters in CSR form: cluster c holds the marks
 * clu_mark[clu_ptr[c] .. clu_ptr[c+1]), each in 0..nk-1; a mark may sit in several clusters, a
 * cluster may be empty, n_clu = 0 skips the cluster outputs.  Outputs (f64, each may be NULL):
 *   contrib[n_models, n, nk], total[n_models, n], prop[n_models, n, nk],
 *   clu[n_models, n, n_clu], clu_prop[n_models, n, n_clu].
 * Arithmetic, every product and sum rounded on its own (no FMA):
 *   A[k], R[k]    the alt / ref features of mark f at decay row k, bitwise what
 *                 expecto_variant_reduce_lut stores at [v, k*nfeat + keep[f]];
 *   D[k]          A[k] - R[k];
 *   contrib       w[m][0*nk+f]*D[0] + w[m][1*nk+f]*D[1] + ... + w[m][9*nk+f]*D[9], left to right;
 *   total         S(contrib[m,v,0..nk-1]);
 *   clu[c]        S(contrib[m,v,mark]) over the cluster's marks in clu_mark order;
 *   prop          contrib / total;   clu_prop[c] = clu[c] / S(clu[m,v,0..n_clu-1])
 * (IEEE divisions: a zero denominator gives nan or inf).  S(x_0 .. x_{c-1}) is one fixed order
 * that depends on c alone: p[l] = x_l + x_{l+64} + x_{l+128} + ... left to right for l = 0..63
 * (-0.0 where there is no term), then p[l] += p[l+s] for l < s, for s = 32, 16, 8, 4, 2, 1;
 * S = p[0]; S of nothing is +0.0.  No atomics: results do not depend on n, n_models or the grid.
 * 8 * (10*n_shift + nk + n_clu + 2) bytes of LDS must fit 160 KiB, else EXPECTO_EINVAL. */
int expecto_variant_contrib(const float* eff_ref, const float* eff_alt, const long long* dist,
                            const uint8_t* strand_plus, const int* shifts, int n_shift, int n, int nfeat,
                            const double* exp_lut, int lut_len, const int* keep, int nk, const double* w, int n_models,
                            const int* clu_ptr, const int* clu_mark, int n_clu, double* contrib, double* total,
                            double* prop, double* clu, double* clu_prop, void* stream);

/* Shift reduction of per-sequence window predictions (fwd and rc [n, n_shift, nfeat] f32, DEVICE)
 * with exp-decay weights [10, n_shift] f64 into float64 features, shifts summed in order.
 * flags bit 0 (EXPECTO_REDUCE_F64AVG): average fwd/rc in float64 (numpy on float64 prediction
 * arrays, geuvadis_*.py) instead of 0.5f*(a+b) in float32 (compute_expecto_features.py:123);
 * bit 1 (EXPECTO_REDUCE_LEGACY20030): out[n, 10, nfeat+1] with a zero column ahead of each
 * decay block ("backwards compatibility" layout, geuvadis_sed_for_top_eqtls.py:112-120),
 * else out[n, 10, nfeat]. */
#define EXPECTO_REDUCE_F64AVG 1
#define EXPECTO_REDUCE_LEGACY20030 2
int expecto_shift_reduce(const float* fwd, const float* rc, const double* weights, int n_genes, int n_shift, int nfeat,
                         int flags, double* out, void* stream);

/* ExPecto expression scoring with an xgboost gblinear model (predict.py:150-166;
 * xgboost 0.7 GBLinear::Pred): out[m] = init + sum_j float32(X[m*ld + cols[j]]) * w[j],
 * summed in float32 in column order with every product and sum rounded separately;
 * init = float32(bias + base_score).  X: float64 feature rows (DEVICE), cols: int32[ncols]
 * (the keep-mask column map of predict.py:137-145), w: float32[ncols]. */
int expecto_gblinear_predict(const double* X, long long n, long long ld, const int* cols, int ncols, const float* w,
                             float init, float* out, void* stream);

/* Training of gblinear / reg:linear models (xgboost 0.7 GBLinear::DoBoost with nthread=1, the
 * arithmetic of DESIGN.md "Training gblinear models"): cyclic coordinate descent, float32 state,
 * double sums over rows in a fixed order, no atomics -- a model's bits do not depend on the batch
 * it is trained in.  X is the float32 feature matrix held COLUMN-major, feature j at X + j*ld
 * (ld >= n), shared by the n_models models of a call; model m has labels y + m*y_stride, row
 * weights h + m*h_stride (h NULL = ones; a stride of 0 shares one vector: a bootstrap replicate
 * is its draw counts as h), weights w + m*(num_feature+1) with the bias last (the .save order)
 * and the workspace sh + m*num_feature.  All pointers are DEVICE memory.
 *
 * One call is one boosting round of every model: predict, gradient, bias step, then one pass
 * over the features in order, updating w in place (zero w before the first round).  first != 0:
 * the call also computes every feature's hessian sum into sh; later rounds (first = 0, same X and
 * h) read it.  pred (may be NULL): [n_models, n], receives the predictions the round STARTED
 * from, i.e. those of the weights the previous round left.  One workgroup holds a model's
 * gradient and row weights on chip for the whole pass: n <= EXPECTO_GBLINEAR_TRAIN_MAX_ROWS
 * (EXPECTO_EINVAL above it; geneanno.csv has 24,338 genes). */
#define EXPECTO_GBLINEAR_TRAIN_MAX_ROWS 24576
int expecto_gblinear_train_round(const float* X, long long ld, int n, int num_feature, int n_models, const float* y,
                                 long long y_stride, const float* h, long long h_stride, float* w, double* sh,
                                 int first, double eta, double lambda, double alpha, double lambda_bias,
                                 float base_score, float* pred, void* stream);

/* The same round with hyper-parameters per model: hyper is a DEVICE array [n_models, 4] of doubles,
 * row m = (eta, lambda, alpha, lambda_bias) of model m (a grid of penalties times cross-validation
 * folds is one batch over one X).  Everything else -- arguments, checks, the row cap, the
 * arithmetic and so the bits -- is expecto_gblinear_train_round's: model m of this call equals
 * that entry point run with row m's scalars.  hyper NULL is EXPECTO_EINVAL.  The values are not
 * validated here (a NaN or negative penalty gives that model NaN or diverging weights and leaves
 * every other model of the batch alone); expecto_amd.xgblinear.train checks them. */
int expecto_gblinear_train_round_hp(const float* X, long long ld, int n, int num_feature, int n_models, const float* y,
                                    long long y_stride, const float* h, long long h_stride, float* w, double* sh,
                                    int first, const double* hyper, float base_score, float* pred, void* stream);

/* out[m, i] = float32(bias_m + base_score) + sum_j X[j*ld + i] * w_m[j], in float32 in column
 * order with every product and sum rounded separately (expecto_gblinear_predict's rule on the
 * column-major float32 matrix); w as above, out [n_models, n].  n_models <= 65535. */
int expecto_gblinear_predict_cols(const float* X, long long ld, int n, int num_feature, int n_models, const float* w,
                                  float base_score, float* out, void* stream);

/* out[m] = sqrt(sum_i h_i * (y_i - pred[m, i])^2 / sum_i h_i) (xgboost's rmse: the square and its
 * product with h in float32, both sums in double); pred [n_models, n], y / h and their strides as
 * above, out float64[n_models]. */
int expecto_gblinear_rmse(const float* pred, const float* y, long long y_stride, const float* h, long long h_stride,
                          int n, int n_models, double* out, void* stream);

/* Ward clustering of the chromatin marks over the training genes (interpret_features.py:99-120,
 * interpret_features_grouped.py:103-146: sklearn's AgglomerativeClustering, i.e. scipy's pdist and
 * its NN-chain Ward linkage), in two steps.
 *
 * Distances, on the device: X is n points of d dimensions, row-major with row stride ld >= d (DEVICE);
 * out (DEVICE) receives the n(n-1)/2 Euclidean distances in scipy's condensed order, pair (i < j) at
 * n*i - i*(i+1)/2 + (j-i-1).  Per pair: s = 0; for k = 0..d-1 in order t = X[i,k] - X[j,k],
 * s = s + t*t (product and sum rounded separately, no FMA); out = sqrt(s) correctly rounded -- the
 * loop of scipy.spatial.distance.pdist, so the bits are scipy's.  The padding X[., d..ld-1] is never
 * read.  n < 2 writes nothing; d = 0 writes +0.0 everywhere.  n <= 2097152. */
int expecto_pairwise_euclidean(const double* X, long long n, long long d, long long ld, double* out, void* stream);

/* Linkage, on the HOST (no device call): scipy.cluster.hierarchy.linkage(condensed, 'ward') bit for
 * bit.  condensed: the n(n-1)/2 distances in HOST memory, overwritten.  Merge i (ascending height,
 * ties in NN-chain order) joins clusters children[2i] < children[2i+1] (ids < n are points, n + m is
 * the cluster merge m made) at heights[i] into sizes[i] points.  n < 2, a NaN distance or a point
 * with no finite distance to any other is refused (EXPECTO_EINVAL). */
int expecto_ward_linkage(double* condensed, int n, int* children, double* heights, int* sizes);

/* Silhouette of the cuts of one tree (interpret_features_grouped.py:120-144: silhouette_score for
 * every n_clusters), from the distances above.  d(i,j) is expecto_pairwise_euclidean's distance,
 * d(i,i) = +0.0.  The arithmetic is fixed:
 *   node sum   S[v,i] = ((+0.0 + d(i,j1)) + d(i,j2)) + ... over the members j1 < j2 < ... of node v in
 *              the order the list gives them (the caller lists them ascending): one sequential float64
 *              chain per (v, i), every add rounded -- np.bincount(labels, weights=D[i]) for that
 *              cluster.  A parent's sum is never formed from its children's.  j == i adds +0.0, which
 *              changes nothing: no sum is ever -0.0.
 *   per cut and point, `own` being the cut's node that holds i:
 *              a = S[own,i] / (|own| - 1);  b = min over the cut's other nodes v of S[v,i] / |v|;
 *              s = (b - a) / max(a, b);  a NaN s (a singleton's 0/0, or a = b = 0) becomes +0.0.
 *              Both divisions are IEEE float64 divisions; nothing is contracted or reassociated.
 * With the members ascending the samples equal sklearn.metrics.silhouette_samples(squareform(pdist(X)),
 * labels, metric='precomputed') bit for bit; the score of a cut is the caller's mean of its row.
 * No atomics: two identical calls give identical bits.  2 <= n <= 1048576 everywhere (EXPECTO_EINVAL
 * otherwise).  Offsets are int64 and are passed twice, in HOST memory (checked here) and in DEVICE
 * memory (read by the kernel, which clamps them to the array's length).
 *
 * expecto_square_distances: condensed [n(n-1)/2] -> square [n, n] (both DEVICE), both triangles and a
 * +0.0 diagonal: the layout in which every member row is contiguous over the points.
 *
 * expecto_silhouette_node_sums: dist is the square matrix (square != 0) or the condensed one
 * (square == 0); same bits.  Node v's members are members[node_ptr[v] .. node_ptr[v+1]) (DEVICE int32;
 * an entry outside [0, n) is passed over).  S (DEVICE) float64 [n_nodes, n].  n_nodes = 0 writes nothing
 * and succeeds.  Refused: node_ptr[0] != 0, decreasing offsets, a node of more than n members.
 *
 * expecto_silhouette_cuts: cut c's nodes are active[cut_ptr[c] .. cut_ptr[c+1]) (DEVICE int32 row
 * indices of S), own [n_cuts, n] (DEVICE int32) the row of S that holds point i in cut c, sizes
 * (DEVICE int32 [n_nodes]) the member counts.  samples (DEVICE) float64 [n_cuts, n].  A row index
 * outside [0, n_nodes) is passed over (as `own`: s = +0.0).  n_cuts = 0 writes nothing and succeeds.
 * Refused: a cut of fewer than 2 or more than n - 1 nodes, cut_ptr[0] != 0, decreasing offsets. */
int expecto_square_distances(const double* condensed, long long n, double* square, void* stream);
int expecto_silhouette_node_sums(const double* dist, int square, long long n, const long long* node_ptr_host,
                                 const long long* node_ptr, const int* members, long long n_nodes, double* S,
                                 void* stream);
int expecto_silhouette_cuts(const double* S, long long n, long long n_nodes, const int* sizes,
                            const long long* cut_ptr_host, const long long* cut_ptr, const int* active, const int* own,
                            long long n_cuts, double* samples, void* stream);

/* Truncated SVD of the tf-idf mark tracks (svd.py:58-85, svd_transform.py:49-81), by the float64 Gram
 * matrix of the tf-idf rows; its eigenproblem is the caller's (expecto_amd/svd.py, on the host).
 *
 * Shared by the four entry points.  D (DEVICE) is one chunk of n columns of the track matrix as the
 * per-gene files hold them: float32 [n, ld], marks contiguous.  keep_idx (DEVICE) int32[m]: the kept
 * marks, distinct, in any order, every entry in [0, ld) (not checked; ld >= m is).  x[n,i] =
 * D[n, keep_idx[i]]; every other element of D is never read.  All arithmetic is float64:
 *   c_n = sum_i x[n,i] (i ascending), idf_n = log(m / (1 + c_n)), r_i = sum_n x[n,i], t[n,i] = x[n,i] idf_n.
 * No atomics: every sum has a fixed order, so two identical calls give identical bits.  n = 0 or
 * m = 0 (or k = 0) is a no-op that writes nothing.  m <= 1048576.
 *
 * expecto_tfidf_stats writes idf[n] and adds the chunk's row sums into rowsum_acc[m].  No scratch: a
 * workgroup owns 16 marks, each of its 16 lanes per mark adds the columns y, y+16, ... in ascending
 * order, and the 16 partial sums are added in ascending y before the one add into rowsum_acc.
 *
 * expecto_tfidf_gram: H_acc[m,m] += sum_n t[n,:]^T t[n,:], the full symmetric matrix (both triangles
 * get the same bits), on v_mfma_f64_16x16x4_f64.  The columns are split into
 * expecto_tfidf_gram_parts(m, n) contiguous parts; each writes its 64 x 64 upper-triangle tiles to
 * `workspace` (DEVICE, at least expecto_tfidf_gram_workspace(m, n) bytes, 8-byte aligned), and a
 * second kernel adds the parts in ascending order into H_acc.  Both sizes are pure host functions
 * (0 for an empty or refused shape).
 *
 * expecto_tfidf_project: out[c, n] = (float)(idf_n * sum_i P[c,i] x[n,i]) for c < k, P float64 [k, m],
 * out float32 with row stride ld_out >= n; the sum in float64 over i ascending, rounded once.
 *
 * expecto_tfidf_transform: X_acc[i, c] += sum_n x[n,i] idf_n V[c,n], V float32 [k, n] with row stride
 * ld_v >= n, X_acc float64 [m, k]; columns split and reduced as the Gram's, with
 * expecto_tfidf_transform_parts / _workspace(m, k, n). */
int expecto_tfidf_stats(const float* D, long long n, long long ld, const int* keep_idx, int m, double* idf,
                        double* rowsum_acc, void* stream);
int expecto_tfidf_gram_parts(int m, long long n);
size_t expecto_tfidf_gram_workspace(int m, long long n);
int expecto_tfidf_gram(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                       double* H_acc, void* workspace, size_t workspace_bytes, void* stream);
int expecto_tfidf_project(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                          const double* P, int k, float* out, long long ld_out, void* stream);
int expecto_tfidf_transform_parts(int m, int k, long long n);
size_t expecto_tfidf_transform_workspace(int m, int k, long long n);
int expecto_tfidf_transform(const float* D, long long n, long long ld, const int* keep_idx, int m, const double* idf,
                            const float* V, long long ld_v, int k, double* X_acc, void* workspace,
                            size_t workspace_bytes, void* stream);

/* k-means of the marks' SVD coordinates (cluster_and_viz.py:45-58: KMeans(n_clusters=k).fit(X), and the
 * commented-out elbow sweep over k), as P independent problems on one matrix per call.  X (DEVICE) is
 * float64 [n, d] with row stride ld >= d; the padding is never read.  Every problem of a call runs at
 * the same time, one workgroup each, and neither kernel returns to the host between seeding steps or
 * iterations.  Supported: 1 <= n <= 4096, 1 <= d <= 128, 1 <= k <= min(n, 512), 1 <= T <= 8,
 * 0 <= P <= 1048576; everything else is EXPECTO_EINVAL with a message.  P = 0 writes nothing and
 * succeeds, whatever the pointers are.
 *
 * Problem tables.  A call's problems are the rows of an int64 table [P, 8], passed twice with the same
 * contents: in HOST memory (checked here) and in DEVICE memory (read by the kernel, which passes over
 * a row that does not fit the checked sizes).  Columns of a seeding row:
 *   0 k   1 first (the first centre's point index)   2 T (trials per step; sklearn's 2 + int(ln k))
 *   3 offset of the problem's uniforms in u (float64 elements)   4 offset of its k indices in idx
 *   5 offset of its k centres in `centres`, in rows of d
 * and of a Lloyd row:
 *   0 k   1 max_iter (>= 1)   2 offset of its k initial centres in init, in rows of d
 *   3 offset of its k centres in `centres`, in rows of d   4 offset of its n labels in labels
 * Columns not named are ignored.  Every offset column starts at 0 in row 0, and row p + 1's block
 * starts at or after the end of row p's (refused otherwise: not 0, decreasing, overlapping).  Also
 * refused: k > n, first outside [0, n), ld < d, a null pointer with P > 0, a workspace smaller than
 * expecto_kmeans_workspace(n, d, max k, max T, P) bytes (a pure host function that covers either
 * call; 0 for a refused shape) or not 8-byte aligned.
 *
 * The arithmetic is fixed.  All of it is float64, products and sums rounded separately (no FMA), no
 * atomics: two identical calls give identical bits, and a problem's bits depend neither on the other
 * rows of the table nor on the launch geometry.
 *   d2(x, c):  s = +0.0; for j = 0..d-1 in order t = x[j] - c[j], s = s + t*t.
 *   sequential sum of a[0..m):  s = +0.0, then s = s + a[i] for i ascending (np.cumsum(a)[-1],
 *     np.add.at): one chain of rounded adds, never a tree.
 *
 * expecto_kmeans_plusplus: sklearn's greedy k-means++ with the caller's random numbers.  u (DEVICE):
 * per problem float64 [k-1, T] uniforms in [0, 1).  closest[i] = d2(X[i], X[first]), pot = sequential
 * sum of closest.  Step c = 1..k-1: cum = the sequential prefix sums of closest; for t < T
 * cand[t] = min(first i with cum[i] >= u[c-1,t]*pot, n-1) (np.searchsorted left, clipped);
 * dc[t][i] = min(closest[i], d2(X[i], X[cand[t]])), pots[t] = sequential sum of dc[t]; the winner is
 * the first t of minimal pots[t]; pot = pots[t], closest = dc[t], idx[c] = cand[t].  idx[0] = first.
 * Outputs (DEVICE): idx int32, the k chosen point indices; centres float64 [k, d], copies of those rows.
 *
 * expecto_kmeans_lloyd: sklearn's _kmeans_single_lloyd.  tol (DEVICE) float64 [P], absolute; init
 * (DEVICE) float64, per problem [k, d].  One iteration:
 *   E-step      label[i] = the lowest c of minimal d2(X[i], C[c]); dist[i] that minimum.
 *   relocation  the e clusters without a label, ascending, receive the e points of largest dist in
 *               descending order, equal dist to the lower point index; such a point counts for its new
 *               cluster and not for its old one in this M-step only; label is unchanged by it.
 *   M-step      sum[c][j] = +0.0, then + X[i][j] over the cluster's members in ascending i;
 *               C_new[c] = sum[c] / (double)count[c] (IEEE division); a cluster still empty keeps its centre.
 *   shift       the sequential sum over (c, j) row-major of (C_new - C)^2;  then C = C_new.
 *   stop        strictly if label equals the previous iteration's (none before the first); else if
 *               shift <= tol; else continue, up to max_iter iterations.
 * After a stop that was not strict one more E-step runs against the final centres.  Outputs (DEVICE):
 * labels int32 [n] per problem, centres float64 [k, d] per problem, inertia float64 [P] = the
 * sequential sum over i of d2(X[i], C[label[i]]) against the final centres, n_iter int32 [P] = the
 * iterations run. */
size_t expecto_kmeans_workspace(long long n, long long d, long long k_max, long long t_max, long long P);
int expecto_kmeans_plusplus(const double* X, long long n, long long d, long long ld, long long P,
                            const long long* prob_host, const long long* prob, const double* u, int* idx,
                            double* centres, void* workspace, size_t workspace_bytes, void* stream);
int expecto_kmeans_lloyd(const double* X, long long n, long long d, long long ld, long long P,
                         const long long* prob_host, const long long* prob, const double* tol, const double* init,
                         int* labels, double* centres, double* inertia, int* n_iter, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Exact t-SNE of the marks' SVD coordinates into two dimensions (cluster_and_viz.py:60-66:
 * TSNE(n_components=2, random_state=0).fit_transform(X)), as sklearn's method='exact' computes it:
 * the affinities once, then the descent in calls of n_iter iterations that the host chains.
 * Supported: 2 <= n <= 4096, 1 <= d <= 128, 0 < perplexity < n; everything else is EXPECTO_EINVAL
 * with a message, as are ld < d, a null pointer, a non-finite exaggeration, momentum or
 * learning_rate, n_iter outside [0, 2^31), and a workspace smaller than expecto_tsne_workspace(n)
 * bytes (a pure host function that covers either call; 0 for a refused n) or not 8-byte aligned.
 * All pointers but the workspace's size are DEVICE memory.
 *
 * The arithmetic is fixed.  All of it is float64, products and sums rounded separately (no FMA), no
 * atomics; / and sqrt are IEEE.  Two identical calls give identical bits, whatever the launch
 * geometry.  Only exp and log (the bisection's p and H, the error) are the device library's and
 * differ from another library's by ulps.
 *   wave-order sum of a[0..m):  (1) lane l of 64 computes s_l = +0.0, then s_l = s_l + a[j] for
 *     j = l, l + 64, ... ascending;  (2) for w = 32, 16, 8, 4, 2, 1 in that order, s_l = s_l + s_{l+w}
 *     for every l < w;  (3) the sum is s_0.
 *   Every sum below is in wave order.  A sum "over j" belongs to row i, and its term for j = i is +0.0.
 *
 * expecto_tsne_affinities: sklearn's _joint_probabilities with _binary_search_perplexity, on float64
 * distances (sklearn rounds them to float32 first) and with the full matrix for its condensed one.
 * X is float64 [n, d] with row stride ld >= d; the padding is never read.
 *   D_ij:  s = +0.0; for t = 0..d-1 in order u = x_it - x_jt, s = s + u*u.
 *   Row i, at most 100 steps from beta = 1, beta_min = -inf, beta_max = +inf:
 *     p_j = exp(-D_ij * beta) (j != i);  S = sum_j p_j, and S = 1e-8 if S == 0;  p_j = p_j / S;
 *     H = log(S) + beta * sum_j (D_ij * p_j);  diff = H - log(perplexity) (the host's log);
 *     stop if |diff| <= 1e-5;  else if diff > 0: beta_min = beta, and beta = 2 * beta while beta_max
 *     is +inf, else beta = (beta + beta_max) / 2;  else beta_max = beta, and beta = beta / 2 while
 *     beta_min is -inf, else beta = (beta + beta_min) / 2.
 *     c_ij = the p_j of the last step taken, c_ii = 0.  beta[i] = the beta of that step, steps[i] =
 *     the steps taken (1..100).
 *   r_i = sum_j (c_ij + c_ji);  T = sum_i r_i;
 *   P_ij = max((c_ij + c_ji) / max(T, eps), eps) for i != j, P_ii = 0, eps = DBL_EPSILON.  P is
 *   symmetric to the bit.
 * Outputs: P float64 [n, n], beta float64 [n], steps int32 [n].
 *
 * expecto_tsne_descend: n_iter iterations of sklearn's _gradient_descent over _kl_divergence with one
 * degree of freedom, enqueued back to back: two launches per iteration and one to close the call, no
 * host synchronisation.  Y, update and gains are float64 [n, 2], read and written, so calls chain:
 * one call of a + b iterations gives the bits of a call of a and then a call of b.  Y is never
 * updated while it is read: an iteration reads one copy and writes the other (the workspace holds
 * the second).  n_iter = 0 succeeds and writes nothing.  One iteration:
 *   pass A   a = y_i0 - y_j0, b = y_i1 - y_j1, num_ij = 1 / (1 + (a*a + b*b));  z_i = sum_j num_ij;
 *            Z = sum_i z_i.
 *   pass B   q = max(num_ij / Z, eps);  t = (exaggeration * P_ij - q) * num_ij;
 *            g_i0 = 4 * sum_j (t * a),  g_i1 = 4 * sum_j (t * b).
 *   update   per element e of [n, 2]:  gain_e = gain_e + 0.2 if update_e * g_e < 0, else gain_e * 0.8;
 *            gain_e = max(gain_e, 0.01);  g_e = g_e * gain_e;
 *            update_e = momentum * update_e - learning_rate * g_e;  y_e = y_e + update_e.
 * stats (float64 [3]) describes the call's last iteration:  stats[1] = sqrt(sum over the 2n entries,
 * row-major, of g_e * g_e) with g after its gain (sklearn's norm is taken there);  stats[2] = Z;  and
 * only if want_error != 0, stats[0] = sum_i (sum_j (P'_ij * log(max(P'_ij, eps) / q_ij))) with
 * P' = exaggeration * P: sklearn's KL divergence, its 2 * sum over i < j taken over the ordered pairs. */
size_t expecto_tsne_workspace(long long n);
int expecto_tsne_affinities(const double* X, long long n, long long d, long long ld, double perplexity, double* P,
                            double* beta, int* steps, void* workspace, size_t workspace_bytes, void* stream);
int expecto_tsne_descend(const double* P, long long n, double exaggeration, double* Y, double* update, double* gains,
                         double momentum, double learning_rate, long long n_iter, int want_error, double* stats,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Louvain clustering of the marks' SVD coordinates (cluster_and_viz_louvain.py: Orange's Louvain(5) on
 * the first 20 coordinates): the k-nearest-neighbour graph with Jaccard weights, then communities of
 * maximal modularity (Blondel et al. 2008, with the resolution of Reichardt and Bornholdt).  Orange and
 * python-louvain were not available: the algorithm is defined here, from the published definitions, and
 * anchored to scikit-learn's NearestNeighbors and networkx's modularity by the tests; agreement with
 * Orange is unmeasured.  All pointers but a workspace's size are DEVICE memory.
 *
 * The arithmetic is fixed.  All of it is float64, products and sums rounded separately (no FMA), no
 * floating-point atomics; / is IEEE.  "Chain" is the sequential sum of the k-means contract: s = +0.0,
 * then s = s + a[i] in the order given.  Two identical calls give identical bits, and a problem's bits
 * depend on nothing but its own inputs.
 *
 * expecto_knn_jaccard.  X float64 [n, d], row stride ld >= d, the padding never read.  Supported:
 * 1 <= n <= 4096, 1 <= d <= 128, 1 <= k <= min(n, 64); everything else, and a null pointer, is
 * EXPECTO_EINVAL with a message and nothing launched.
 *   d2(i, j):  s = +0.0; for c = 0..d-1 in order t = x_ic - x_jc, s = s + t*t (plain multiply and add).
 *   N(i) = the k points j of smallest (d2(i, j), j), i itself a candidate: what
 *     NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X) returns when no distances tie.
 *   nbr int32 [n, k]: N(i) in ascending (d2, j).
 *   w float64 [n, k]: for j = nbr[i, t], c = |N(i) & N(j)| as sets, w[i, t] = (double)c / (double)(2k - c);
 *     0 where j == i.
 *
 * expecto_louvain: P problems over one undirected weighted graph in CSR form: indptr int32 [n + 1],
 * indices int32 [nnz], weights float64 [nnz]; every edge {u, v} is stored in both rows with the same
 * weight, and the input holds no self-loop.  Problem p has the resolution gamma[p] (float64 [P]) and the
 * visiting order perm[p] (int32 [P, n], each row a permutation of 0..n-1).  One wave runs one problem.
 * Supported: 1 <= n <= 4096, 0 <= nnz <= 1048576, 0 <= P <= 65535, 1 <= max_passes <= 1000,
 * 1 <= max_levels <= 64; everything else, a null pointer, a workspace smaller than
 * expecto_louvain_workspace(n, nnz, P) bytes (a pure host function; 0 for a refused shape) or not 8-byte
 * aligned is EXPECTO_EINVAL.  P = 0 writes nothing and succeeds.  The graph and the orders are never seen
 * by the host: a problem whose indptr does not rise from 0 to nnz, or with an index or an order entry
 * outside [0, n), writes only modularity 0, counters 0 and the flag EXPECTO_LOUVAIN_BAD_GRAPH.
 *
 * A level works on a graph whose rows may hold a self-loop entry (v, v), of weight s: the weight inside
 * v, each edge once.
 *   degree      k_v = the chain over row v in row order, the self-loop entry as 2*s;  2m = the chain of
 *               k_v over v ascending.  If 2m == 0 at level 0 every node is its own community:
 *               modularity 0, n_levels 0, n_passes 0, flags 0.
 *   start       every node in its own slot: comm[v] = v, D[v] = k_v.
 *   pass        visit v in perm's order at level 0, in ascending v above it.  old = comm[v];
 *               D[old] = D[old] - k_v.  For every slot c = comm[x] of an entry x != v of row v,
 *               k_vc = the chain of the row's weights towards c in row order; k_v,old = +0.0 if the row
 *               has no such entry.  gain(c) = k_vc - ((gamma * D[c]) * k_v) / 2m.  v goes to the slot of
 *               largest gain, old if it ties for it, else the lowest such slot: to.
 *               D[to] = D[to] + k_v (also when to == old).
 *   Q           lin_v = the chain, in row order, of row v's weights towards x >= v with comm[x] == comm[v];
 *               L_c = the chain of lin_v over the slot's nodes v ascending;
 *               Q = the chain over all slots c ascending, empty ones too, of
 *               L_c / (2m * 0.5) - gamma * ((D[c] / 2m) * (D[c] / 2m)), with D as the passes left it.
 *               This is networkx.community.modularity(G, parts, weight='weight', resolution=gamma).
 *   level       Q is taken once before the first pass of level 0 and after every pass.  Passes end after
 *               a pass that moved no node or raised Q by less than 1e-7, and after max_passes passes
 *               (flag EXPECTO_LOUVAIN_PASS_BOUND unless that pass also met a stop).  A level whose
 *               passes moved no node ends the run.
 *   aggregate   slots are renumbered in ascending order of their smallest node; labels follow.  New
 *               node C's entry towards C' != C is the chain of w(u, x) over C's nodes u ascending and
 *               their rows in order, for comm[x] == C'; its self-loop is the same chain over
 *               comm[x] == C and x >= u, present if that chain has a term.  Rows are in ascending
 *               neighbour id, the self-loop in its place.  Degrees and 2m are taken anew.
 *   run         After aggregating, the run ends if Q rose by less than 1e-7 over the level; after
 *               max_levels levels it ends with the flag EXPECTO_LOUVAIN_LEVEL_BOUND.
 * Outputs: labels int32 [P, n], communities numbered in ascending order of their smallest node;
 * modularity float64 [P], the last Q taken; counters int32 [P, 4]: n_communities, n_levels (the levels
 * aggregated), n_passes (all levels') and flags. */
#define EXPECTO_LOUVAIN_PASS_BOUND 1
#define EXPECTO_LOUVAIN_LEVEL_BOUND 2
#define EXPECTO_LOUVAIN_BAD_GRAPH 4
int expecto_knn_jaccard(const double* X, long long n, long long d, long long ld, long long k, int* nbr, double* w,
                        void* stream);
size_t expecto_louvain_workspace(long long n, long long nnz, long long P);
int expecto_louvain(const int* indptr, const int* indices, const double* weights, long long n, long long nnz,
                    long long P, const double* gamma, const int* perm, long long max_passes, long long max_levels,
                    int* labels, double* modularity, int* counters, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Motif-match enrichment of the top clusters (cluster_analysis_with_fimo.py:126-162: the counting of
 * cluster_contribs_hypergeom), as P problems over one contribution matrix per call.
 *
 * Shared inputs (DEVICE unless said).  contrib: float64 [V, ld], ld >= C, the padding never read; it is
 * copied to the host once, on `stream` and with a wait, and a NaN in a read element is refused.  sets:
 * uint64 [C, W], W = ceil(M / 64): bit m of row c says that motif m is in column c's set; bits at or
 * above M are zero.  A motif may be in several sets.  seq_ptr: int64 [S + 1], passed twice with the same
 * contents, in HOST memory (checked: starts at 0, never decreases) and in DEVICE memory (clamped to the
 * checked length); motif_idx: int32 [seq_ptr[S]], the match entries of sequence s at
 * [seq_ptr[s], seq_ptr[s+1]); an entry outside [0, M) counts nowhere.  An entry may repeat.
 *
 * Problems: an int64 table [P, 4], passed in HOST memory (checked) and in DEVICE memory (a row that
 * does not fit the checked sizes is passed over).  Columns:
 *   0 permutation slot: -1 for none, else j < n_perms: column c of row v holds contrib[v, perms[j, v, c]],
 *     perms uint16 [n_perms, V, C]; an entry >= C reads column c.  Not checked to be a permutation.
 *   1 sid slot j < n_sids: sids int32 [n_sids, V], sids[j, v] the sequence of row v; outside [0, S): none.
 *   2, 3 offset and count of the problem's rows in `rows` (int32 [rows_len], values in [0, V); others are
 *     passed over).  Row lists may overlap or be shared.
 *
 * Per row the columns are ordered by |value| descending, equal magnitudes (+x and -x, zeros) the lower
 * column first; rank 0 is the largest.  Outputs (DEVICE), every one a sum or minimum of integers, so
 * independent of the launch geometry and of the order of the adds:
 *   pos_matches int64 [P, T]  sum over rows of the row's entries whose motif is in the set at rank t
 *   pos_motifs  int64 [P, T]  sum over rows of that set's popcount
 *   neg         int64 [P, 2]  the same two sums for the OR of the sets at the last n_neg ranks
 *   min_rank    int32 [P, C]  the least rank column c takes over the rows; C for a problem without rows
 * A row without a sequence adds to the motif sums only.  workspace: at least
 * expecto_cluster_enrich_workspace(S, C) bytes (a pure host function; 0 for a refused shape), 4-byte
 * aligned: the matches per (sequence, column), which no problem changes, are counted once per call.
 * Refused (EXPECTO_EINVAL, nothing launched): C outside [1, 1024], M outside [1, 32768], n_neg or T
 * outside [1, C], ld < C, V * C or S * C >= 2^31, P > 1048576, more than 2097120 rows in a problem, a
 * slot or row list outside its array, a null pointer, NaN in contrib.  P = 0 or V = 0 launches nothing,
 * writes nothing and succeeds.
 *
 * expecto_hypergeom_sf: out[q] = P(X >= k[q]) for X hypergeometric with population M[q], n[q] marked and
 * N[q] drawn (scipy.stats.hypergeom.sf(k - 1, M, n, N)); int64 inputs, float64 output, all DEVICE, one
 * lane per quadruple.  NaN, as scipy's argument check gives, for M <= 0, a negative n or N, n > M or
 * N > M.  With lo = max(0, N - (M - n)) and hi = min(n, N): 1 for k <= lo, 0 for k > hi.
 * Otherwise the sum of the positive terms i = k .. hi: the term at max(k, mode) as the product of its
 * 2 min(n, N) integer ratios (exponent kept apart; about 1e-13 relative at N = 1e5, where differences
 * of lgamma give 1e-9), its neighbours by the ratio (n-i)(N-i) / ((i+1)(M-n-N+i+1)) upwards and its
 * inverse downwards, each direction until a term no longer changes the sum.  count = 0 succeeds without a launch. */
size_t expecto_cluster_enrich_workspace(long long S, long long C);
int expecto_cluster_enrich(const double* contrib, long long V, long long C, long long ld,
                           const unsigned long long* sets, long long M, const long long* seq_ptr_host,
                           const long long* seq_ptr, const int* motif_idx, long long S, const long long* prob_host,
                           const long long* prob, long long P, const unsigned short* perms, long long n_perms,
                           const int* sids, long long n_sids, const int* rows, long long rows_len, long long n_neg,
                           long long T, long long* pos_matches, long long* pos_motifs, long long* neg, int* min_rank,
                           void* workspace, size_t workspace_bytes, void* stream);
int expecto_hypergeom_sf(const long long* k, const long long* M, const long long* n, const long long* N,
                         long long count, double* out, void* stream);

/* Motif scan of short sequences with FIMO's scoring model (query_fimo_for_predictions.py:43-57), as far as
 * it is documented (Grant, Bailey, Noble 2011); agreement with the `fimo` binary has not been measured.
 *
 * Motifs: pssm int16 [col_ptr[M], 4] (DEVICE), the scaled log-odds entries in 0..100, a row per motif
 * column, the four entries in base-code order (0=A 1=G 2=C 3=T); col_ptr int32 [M + 1], passed twice with
 * the same contents, in HOST memory (checked: starts at 0, widths in [1, 64]) and in DEVICE memory (a
 * motif that does not fit the checked sizes is passed over).  Table of motif m: 100 w + 1 doubles at
 * tables[pv_ptr[m]], pv_ptr[m] = 100 col_ptr[m] + m: the tables lie back to back.
 *
 * expecto_pwm_pvalues: bg_host float64 [4] (HOST, code order, each in (0, 1)).  Writes pv_ptr int64
 * [M + 1] and the tables (both DEVICE): pv[j] = P(score >= j) of a sequence of w independent letters drawn
 * from bg.  All float64, products and sums rounded separately (no FMA), one workgroup per motif:
 *   pdf = [1.0]; per column i = 0..w-1: new[0..100(i+1)] = +0.0, then for k ascending and the letters in
 *   alphabet order (A C G T) new[k + s[i][a]] += pdf[k] * bg[a].  The kernel gathers: new[j] is +0.0 plus
 *   its up to four terms in that same order (entry descending, then alphabet order).
 *   pv[100 w] = pdf[100 w], pv[j] = pv[j + 1] + pdf[j] downwards, one chain; then pv = min(pv, 1.0), and
 *   pv[0] = 1.0: every score is >= 0, and the clip alone leaves a chain that ends a few ulp below 1 there.
 * pssm is copied to the host once, on `stream` and with a wait, for the entry check.  Refused
 * (EXPECTO_EINVAL, nothing launched or written): a width outside [1, 64], a decreasing col_ptr, an entry
 * outside 0..100, tables_len < 100 col_ptr[M] + M, a background frequency outside (0, 1), a null pointer.
 * M = 0 succeeds without a launch.
 *
 * expecto_pwm_scan: codes uint8 [S, ld] (DEVICE), ld >= L, columns at or above L never read; a code >= 4
 * is no base.  overlap int32 [S] (DEVICE): c >= 0 keeps the windows that cover position c (0-based), a
 * negative c all windows.  Window start p of a motif of width w is admissible when 0 <= p, p + w <= L,
 * p <= c <= p + w - 1 (c >= 0), and no code in the window is >= 4.  Scores are integer sums:
 *   '+': sum_i s[i][seq[p + i]];   '-': sum_i s[w-1-i][3 - seq[p + i]] (the reverse-complement motif read
 *   on the given strand).
 * Outputs (DEVICE, [S, M] row-major), the maximum score, equal scores to the smaller p, then to '+':
 *   score int32 (-1: no admissible window), start int32 (0-based p, or -1), strand uint8 (0 '+', 1 '-'),
 *   pvalue float64 = tables[pv_ptr[m] + score] (NaN without a window): the one non-integer step, a lookup;
 *   both strands read the forward matrix's table.
 * Plain vector stores, no atomics: the bits depend on nothing but the pair's own inputs.  A workgroup takes
 * 64 sequences x 16 motifs.  Refused: L outside [1, 256], ld < L, a width outside [1, 64], a decreasing
 * col_ptr, M > 1048560, tables_len < 100 col_ptr[M] + M, a null pointer.  S = 0 or M = 0 succeeds without a
 * launch. */
int expecto_pwm_pvalues(const short* pssm, const int* col_ptr_host, const int* col_ptr, long long M,
                        const double* bg_host, double* tables, long long* pv_ptr, long long tables_len, void* stream);
int expecto_pwm_scan(const unsigned char* codes, long long S, long long L, long long ld, const int* overlap,
                     const short* pssm, const int* col_ptr_host, const int* col_ptr, long long M, const double* tables,
                     const long long* pv_ptr, long long tables_len, int* score, int* start, unsigned char* strand,
                     double* pvalue, void* stream);

/* Motif similarity clustering (cluster_by_pwm.py writes cluster_motifs.jaspar for RSAT matrix-clustering,
 * which is not part of this project): every pair of motifs compared at every offset on both strands, an
 * average-linkage tree of the distances and its cut by two thresholds.  The arithmetic follows RSAT's
 * published definitions of cor, Ncor and average linkage and is fixed below; agreement with RSAT itself
 * has not been measured.
 *
 * expecto_pwm_compare.  freq float64 [col_ptr[M], 4] (DEVICE): the frequencies of all motifs, a row per
 * motif column, the four entries in alphabet order A C G T; every row sums to 1 up to rounding, so the
 * mean over any set of whole columns is 0.25 and the centred value is a = f - 0.25.  col_ptr int32
 * [M + 1], passed twice with the same contents, in HOST memory (checked: starts at 0, widths in [1, 64])
 * and in DEVICE memory (a motif that does not fit the checked sizes is passed over, and so are its pairs).
 * For the pair (A, B) = motifs (i < j) of widths wA, wB:
 *   strands    D compares A with B, R with B_rc[c][b] = B[wB-1-c][3-b];
 *   offsets    o is the column of A under column 0 of B (or B_rc); need = min(min_w, wA, wB); o runs from
 *              -(wB - need) to wA - need; the overlap is A's columns [max(0, o), min(wA, o + wB)), w wide;
 *   sums       num = S a*b, ssa = S a*a, ssb = S b*b over the overlap, A's columns ascending and A C G T
 *              within a column, each sum one chain s = +0.0, s = s + x*y in float64, the product rounded
 *              before the add (no FMA);
 *   scores     cor = num / sqrt(ssa * ssb), or 0 when ssa * ssb == 0 (IEEE / and sqrt);
 *              Ncor = cor * (double)w / (double)(wA + wB - w), evaluated left to right;
 *   best       the largest Ncor; equal Ncor to strand D before R, then to the smaller o.
 * Outputs (DEVICE), M(M-1)/2 entries each, pair (i < j) at scipy's condensed index
 * M i - i(i+1)/2 + (j - i - 1):  cor, ncor float64, the best alignment's;  dist float64 = 1 - Ncor, or 0 if
 * that is negative;  offset int32 = o;  strand int32, 0 for D and 1 for R;  width int32 = w.
 * Plain vector stores, no atomics: a pair's bits depend on nothing but the two motifs and min_w.  A
 * workgroup takes a 16 x 16 tile of pairs of the upper triangle, one lane per pair.  Refused
 * (EXPECTO_EINVAL, nothing launched or written): M outside [0, 4096], min_w < 1, a width outside [1, 64],
 * col_ptr[0] != 0, a decreasing col_ptr, a null pointer with M >= 2.  M < 2 succeeds without a launch.
 *
 * expecto_average_linkage (HOST memory throughout): scipy's linkage(method='average') of n(n-1)/2
 * condensed distances, which are overwritten: the NN-chain algorithm with strict < and the previous chain
 * element preferred, the update d(k, x u y) = (n_x d_kx + n_y d_ky) / (n_x + n_y) evaluated left to right,
 * a stable sort of the merges by height and a union-find relabelling.  Row i of children int32 [n-1, 2],
 * heights float64 [n-1] and sizes int32 [n-1] is the i-th merge by height; it forms cluster n + i out of
 * children[i] (smaller id first).  Refused: n < 2, a NaN distance, a cluster whose every distance is +inf.
 *
 * expecto_linkage_threshold_cut (HOST memory throughout): children as above; cor, ncor float64 [n(n-1)/2].
 * For merge i of the clusters X = children[i][0] and Y = children[i][1], mean_cor[i] is s = +0.0, then
 * s = s + cor[x, y] over X's leaves ascending (outer) and Y's leaves ascending (inner), then
 * s / (double)(|X| |Y|); mean_ncor[i] likewise.  Merge i is accepted when both children are leaves or
 * accepted merges and mean_cor[i] >= min_cor and mean_ncor[i] >= min_ncor.  The clusters are the maximal
 * accepted nodes (a leaf under no accepted merge is its own); labels int32 [n] are 1-based, numbered by
 * ascending smallest member index.  Refused: n < 2, children that do not form a tree (a child outside
 * [0, n + i) or used twice), a null pointer. */
int expecto_pwm_compare(const double* freq, const int* col_ptr_host, const int* col_ptr, long long M, int min_w,
                        double* cor, double* ncor, double* dist, int* offset, int* strand, int* width, void* stream);
int expecto_average_linkage(double* condensed, int n, int* children, double* heights, int* sizes);
int expecto_linkage_threshold_cut(const int* children, int n, const double* cor, const double* ncor, double min_cor,
                                  double min_ncor, int* labels, double* mean_cor, double* mean_ncor);

/* Scores of trained models and statistics of a bootstrap batch (train_susztak.py:146-181,
 * plot_bootstrapped_coefficients.py:52-76).  All pointers are DEVICE memory, strides are in elements, and a
 * refused call (EXPECTO_EINVAL) launches and writes nothing.
 *
 * expecto_rank2_f32 / _f64: x holds P rows of n values, row p at x + p*stride; out int32 [P, n] (contiguous)
 * receives out[p, i] = 2 * #{j : x_j < x_i} + #{j : x_j == x_i} + 1, twice scipy's rankdata(method='average')
 * as an exact integer.  The ranks are counted, not sorted: one thread owns one i, the row streams through
 * LDS, the grid is (ceil(n / 256), P).  The comparisons are IEEE < and ==: -0.0 ties with 0.0, and a NaN
 * compares false with everything (its own doubled rank is 1, and it does not move the others').
 * 0 <= n <= EXPECTO_METRICS_MAX_ROWS, 0 <= P <= 65535; n = 0 or P = 0 succeeds without a launch.
 *
 * expecto_model_metrics: out float64 [P, 3] = (pearson, spearman, r2) of model p's predictions
 * pred + p*pred_stride (float32 [n]) against the labels y + p*y_stride (float64 [n]; y_stride == 0: every
 * model shares one label row).  rank_pred int32 [P, n] and rank_y int32 [P, n] (or [n] when y_stride == 0)
 * are the doubled ranks of the same rows from expecto_rank2_*.  One workgroup of 256 threads per model.
 *   spearman = double(n Sab - Sa Sb) / sqrt(double(n Saa - Sa^2) * double(n Sbb - Sb^2)) from exact int64 sums
 *   of the doubled ranks; a doubled rank is at most 2n, so every term is at most 4 n^4 = 2^62 at n = 32768
 *   (below even the cruder bound n^2 (2n+1)^2 ~ 4.6e18 < 2^63).  A zero denominator gives NaN, as scipy does
 *   for a constant input.
 *   pearson and r2 in float64, two passes, pred widened exactly, no FMA.  Every sum: thread t adds elements
 *   t, t+256, ... in ascending order onto +0.0, then the 256 partials fold by p[i] = p[i] + p[i+w] for i < w,
 *   w = 128 ... 1.  mx = Sx / double(n), my likewise; sxy = S (x-mx)(y-my), sxx, syy, ssr = S (y-x)^2;
 *   pearson = sxy / sqrt(sxx * syy) clipped to [-1, 1]; r2 = 1 - ssr / syy, and for syy == 0 sklearn's
 *   force_finite: 1.0 if ssr == 0 else 0.0.
 * A NaN anywhere in a model's pred or y makes its three outputs NaN.  2 <= n <= EXPECTO_METRICS_MAX_ROWS,
 * P >= 0 (P = 0 succeeds without a launch).
 *
 * expecto_bootstrap_coef_stats: W float64 [B, F] row-major with row stride ld >= F, the coefficients of B
 * bootstrap models; w_main float64 [F], the main model's.  One thread per coefficient walks the models in
 * ascending order (numpy's order for an axis=0 reduction), no FMA:
 *   mean = S w / B; se = sqrt(S (w - mean)^2 / (B - 1)); z = w_main / se; cv = se / |mean|   (float64 [F] each)
 * with IEEE division by zero kept (inf or NaN, as numpy gives).  2 <= B <= 4096, F >= 0. */
#define EXPECTO_METRICS_MAX_ROWS 32768
int expecto_rank2_f32(const float* x, long long stride, int n, int P, int* out, void* stream);
int expecto_rank2_f64(const double* x, long long stride, int n, int P, int* out, void* stream);
int expecto_model_metrics(const float* pred, long long pred_stride, const double* y, long long y_stride,
                          const int* rank_pred, const int* rank_y, int n, int P, double* out, void* stream);
int expecto_bootstrap_coef_stats(const double* W, long long ld, int B, int F, const double* w_main, double* mean,
                                 double* se, double* z, double* cv, void* stream);

/* In-silico saturation mutagenesis: every SNV of a region, enumerated and scored on the device (the
 * reference has no script for it; it would be a VCF of 3 L SNVs through chromatin.py,
 * make_closest_genes_file.py and predict.py once per tissue model).  All pointers are DEVICE memory unless
 * noted; a refused call (EXPECTO_EINVAL) launches and writes nothing.
 *
 * expecto_ism_variants: the SNVs of the L genome offsets start .. start + L - 1 (0 <= start,
 * start + L <= genome_len; code alphabet of expecto_variant_windows: 0=A 1=G 2=C 3=T 4=zero column).  3 L
 * slots, slot 3*p + j of position p: var_off (int64) = start + p; ref_code = genome[start + p]; alt_code = the
 * j-th of the base codes 0..3, in code order, that is not ref_code; valid (uint8) = 1.  A position whose code
 * is not a base gets valid = 0 and alt_code = ref_code in its three slots: its windows are no-ops and nothing
 * downstream needs compaction.  Slots are fixed (no atomics, no scan): the output does not depend on the grid.
 *
 * expecto_ism_score: expression predictions of both alleles of every slot for n_models gblinear models at
 * once, without the [n, 10*nfeat] float64 feature matrices.  y_ref, y_alt: float32 chromatin rows of both
 * strands as expecto_beluga_forward_segment_pairs writes them for rows="shift": row s*strand_stride + j*n + v
 * for strand s, shift j (n_shift of them, the order of `shifts`) and slot v (n of them, n % 3 == 0, three per
 * position); strand_stride >= n_shift*n.  dist[n] (pos - TSS, int64), shifts, exp_lut, lut_len: as
 * expecto_variant_reduce_lut; strand_plus: HOST scalar, the gene's strand (one gene per call).  keep[nk]: the
 * kept mark columns, ascending, each in 0..nfeat-1.  w: float32 [10*nk, n_models], model m's weight of feature
 * column c = k*nk + f at w[c*n_models + m] (the models of a wave read one contiguous run per column);
 * init[n_models]: float32(bias + base_score) of each model.  valid[n]: as expecto_ism_variants gives it.
 * Outputs: alt_pred float32 [n_models, n]; ref_pred float32 [n_models, n/3], one per position, from the ref
 * rows and the distance of the position's first slot (the three slots of a position hold the same ref window);
 * sed float64 [n_models, n] = (double)alt_pred - (double)ref_pred[position].  An invalid slot gets NaN in
 * alt_pred and sed; a position with three invalid slots gets NaN in ref_pred.
 * Arithmetic: bitwise what the unfused chain gives on the same rows -- expecto_fwd_rc_average of each allele,
 * expecto_variant_reduce_lut (float64, shifts summed in order from the first term, a distance bin
 * fl >= lut_len through the device exp), expecto_gblinear_predict per model over the columns k*nfeat + keep[f]
 * (float32, init first, column order, every product and sum rounded on its own, no FMA).  One workgroup per
 * position and 256 models; no atomics: results do not depend on n_models, n or the grid.
 * 240*n_shift + 16*nk bytes of LDS must fit 160 KiB and n_shift <= 819, else EXPECTO_EINVAL.
 *
 * expecto_ism_summary: potential[m] = S(|sed[m, .]|) and direction[m] = S(sed[m, .]) over the n slots in slot
 * order (float64 [n_models] each), S the fixed order of expecto_variant_contrib; an invalid slot's term is
 * -0.0, which changes no sum.  One wave per model. */
int expecto_ism_variants(const uint8_t* genome, long long genome_len, long long start, int L, long long* var_off,
                         uint8_t* ref_code, uint8_t* alt_code, uint8_t* valid, void* stream);
int expecto_ism_score(const float* y_ref, const float* y_alt, long long strand_stride, const long long* dist,
                      int strand_plus, const int* shifts, int n_shift, int n, int nfeat, const double* exp_lut,
                      int lut_len, const int* keep, int nk, const float* w, const float* init, int n_models,
                      const uint8_t* valid, float* alt_pred, float* ref_pred, double* sed, void* stream);
int expecto_ism_summary(const double* sed, const uint8_t* valid, int n_models, int n, double* potential,
                        double* direction, void* stream);

/* Empirical significance of effects against a background (e-values).  These definitions are this project's:
 * the reference has no script for them and no published table is reproduced.  All pointers are DEVICE memory
 * unless noted; a refused call (EXPECTO_EINVAL) launches and writes nothing.
 *
 * Inputs.  bg float32 [C, B]: per mark c the B background effect magnitudes sorted ascending, no NaN,
 * 1 <= B <= 2^31 - 2.  x float32 [n, >= max(cols) + 1] with row stride x_stride (elements).  cols[nc]: ascending
 * mark indices in 0..C-1, 1 <= nc <= C, given twice: cols_host (HOST memory) is checked -- ascending, in range,
 * x_stride >= cols_host[nc-1] + 1 -- before any launch, cols is the same list on the device and the caller's
 * duty to keep equal.  With a = |x[v, cols[j]]|:
 *   ge[v, j]     = #{b : bg[cols[j], b] >= a}, int32 [n, nc] contiguous.  Exact; ties count; a = +inf counts the
 *                  background's infinities; a NaN query gives -1.
 *   e[v, j]      = (ge + 1) / (B + 1) in float64 (the add-one form of permutation_null.tsv);
 *   nlog[v, j]   = lut[ge[v, j]], lut[k] = -log10((k + 1) / (B + 1)) a float64 table of B + 1 entries that the
 *                  HOST computes and uploads (as the exp table of expecto_variant_reduce_lut: the device log
 *                  differs in the last ulp);
 *   mean_nlog[v] = S(nlog[v, 0..nc-1]) / nc, S the fixed order of expecto_variant_contrib;
 *   max_nlog[v]  = the largest nlog[v, j];
 *   top[v]       = the lowest j whose ge[v, j] is the row's smallest;
 *   n_sig[v]     = #{j : ge[v, j] + 1 <= k_alpha}, k_alpha = floor(alpha * (B + 1)) an integer the HOST computes,
 *                  0 <= k_alpha <= B + 1.
 * A variant with a NaN query (a -1 in its ge row) gets NaN in mean_nlog and max_nlog and -1 in top and n_sig.
 * No atomics: every output depends on its own inputs alone, not on n or the grid.
 *
 * expecto_ecdf_tail_counts: a two-level lower bound.  A workgroup of 16 waves owns EXPECTO_ECDF_TILE_COLS = 16
 * columns, one per wave, and keeps of each EXPECTO_ECDF_SPLITTERS = 2048 splitters (every ceil(B / 2048)-th
 * value; the whole column where B <= 2048) in 128 KiB of LDS; |x| passes through a [16][257]-word LDS tile
 * (16 KiB) that transposes 256 variants so that lanes are variants, four per lane side by side.  The first
 * 11 halving steps read LDS, the remaining bit_length(ceil(B / 2048) - 1) read the column (6 at B = 10^5).
 * Column tiles are dealt to the 8 workgroup groups of the XCDs, so the workgroups that share an L2 search the
 * same 16 columns while the variants stream past.  n = 0 succeeds without a launch.
 *
 * expecto_ecdf_summary: one wave per variant reads the ge row (every entry -1 or 0..B, as tail_counts writes
 * them), gathers lut and reduces. */
#define EXPECTO_ECDF_SPLITTERS 2048
#define EXPECTO_ECDF_TILE_COLS 16
int expecto_ecdf_tail_counts(const float* bg, int B, int C, const int* cols_host, const int* cols, int nc,
                             const float* x, long long x_stride, int n, int* ge, void* stream);
int expecto_ecdf_summary(const int* ge, int n, int nc, const double* lut, int B, int k_alpha, double* mean_nlog,
                         double* max_nlog, int* top, int* n_sig, void* stream);

const char* expecto_last_error(void);
const char* expecto_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EXPECTO_HIP_H */
