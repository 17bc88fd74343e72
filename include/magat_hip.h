/* magat_hip.h -- C ABI of libmagat_hip.so (MI355X / gfx950 only).
 *
 * The reference (proroklab/magat_pathplanning) is pure Python/PyTorch and has no FFI of its
 * own, so the "binding a maintainer would add" is a ctypes stub.  Every
 * entry point below names the reference code it replaces.  Conventions:
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only
 *     enqueues work on that stream, never allocates, never synchronises;
 *   - the caller owns every buffer including `workspace` (size from the matching
 *     *_workspace_bytes query; 256-byte aligned);
 *   - return value: MAGAT_OK (0) or a negative MAGAT_ERR_* code; nothing throws.
 * Layout vocabulary: B planning instances, N agents per instance, M = B*N agent rows,
 * G in-features, F out-features per head, K filter taps, P attention heads.
 */
#ifndef MAGAT_HIP_H
#define MAGAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAGAT_OK 0
#define MAGAT_ERR_BAD_SHAPE (-1)   /* non-positive or inconsistent dimensions                */
#define MAGAT_ERR_UNSUPPORTED (-2) /* feature width / mode the gfx950 kernels do not cover   */
#define MAGAT_ERR_WORKSPACE (-3)   /* workspace NULL, misaligned or smaller than required    */
#define MAGAT_ERR_LAUNCH (-4)      /* hipLaunchKernel / hipGetLastError reported a failure   */
#define MAGAT_ERR_NULL (-5)        /* a required pointer is NULL                             */

#define MAGAT_MODE_KEYQUERY 0     /* attentionMode == 'KeyQuery'      graphML.py:1180-1286 */
#define MAGAT_MODE_GAT_MODIFIED 1 /* attentionMode == 'GAT_modified'  graphML.py:713-823   */
#define MAGAT_MODE_GAT_ORIGIN 2   /* attentionMode == 'GAT_origin' (GraphFilterBatchAttentional_Origin, graphML.py:4175-4339,
                                     964-1069, 1939-2002): self-loops added to the GSO (mask = |float(S)+I| > 1e-9), scores
                                     lrelu(a1.Wx_j + a2.Wx_i) without weight_bias, filter taps h[p,f,k,g] = filterWeight[0,k] * W[p,g,f]
                                     (transposed: the reference's permute+reshape, graphML.py:1967-1969).
                                     pack_weights: `taps` = filterWeight (E=1,K), `weight_bias` ignored. */
#define MAGAT_MODE_GNN 3          /* no attention: GraphFilterBatch / BatchLSIGF (graphML.py:5485-5700), the GNN baseline:
                                     z_k = z_{k-1} @ float(S), the edge weights are the GSO VALUES (CSR entry point only,
                                     magat_gnn_forward_csr_f32; P = 1, taps = weight (F,1,K,G), no ReLU inside the layer) */
#define MAGAT_MODE_SIMILARITY 4   /* attentionMode == 'GAT_Similarity' (GraphFilterBatchSimilarityAttentional, graphML.py:4690-4857,
                                     1449-1564, 2095-2179): cosine scores e_ij = (x_i / max(|x_i|, 1e-9)) . (q_j / max(|q_j|, 1e-9)),
                                     q_j = W x_j (no bias, no LeakyReLU) under GAT_origin's mask |float(S)+I| > 1e-9; the filter is
                                     KeyQuery's (full taps (P,F,1,K,G)).  P = 1 and G == F only (the reference's own reshapes need
                                     both).  Pack layout: KeyQuery's; `weight_bias` and `mixer` are ignored.  float32 inference
                                     entry points only.  One launch (gat_small.hip / gat_mid.hip, cosine scores in the G2 epilogue)
                                     for 32 / 64 features on N <= 128 and 128 features on N = 97 .. 105, K = 2 | 3, with the range
                                     guard on: a value beyond the f16 planes' range OR a non-zero row too small for their
                                     resolution (scaled norm below 1 / 8) raises the flag, and the predicated float32 form rewrites
                                     the output.  That form, and every other shape: float32 MFMA maps GEMM, one kernel that
                                     normalises the Q columns of the maps and writes the normalised rows of X into the workspace
                                     (magat_gat_workspace_bytes and the CSR sizes grow by B N G floats), then the KeyQuery graph
                                     kernels on them (128 features beyond 105 agents and N > 128: the generic CSR score and hop
                                     kernels).  The bf16 entry points and magat_gat_train_forward_f32 / _backward_f32 answer
                                     MAGAT_ERR_UNSUPPORTED, as does any call with P != 1 or G != F; training runs through the
                                     pair of its own, magat_gat_train_forward_cos_f32 / _backward_cos_f32 (below). */

int magat_abi_version(void);
/* 0 = release build.  1 = EXPERIMENT build: at least one source was compiled with timing-experiment switches (*_WHATIF_*:
 * phases of a kernel replaced by register sinks - the results are WRONG by design; tools/whatif_*.sh).  Such a source only
 * compiles under -DMAGAT_EXPERIMENT_BUILD, which also marks the library here; the Python binding refuses to load a library
 * whose flavor is not 0 unless MAGAT_ALLOW_EXPERIMENT_BUILD=1 (the probe scripts set it). (ABI 4) */
int magat_build_flavor(void);
const char* magat_error_string(int code);

/* Options.  Every tunable of the library lives in one table that is seeded from the environment (MAGAT_<NAME>) ONCE, at
 * first use, and is read / changed through these calls afterwards; nothing on the launch path calls getenv.  `name` with
 * or without the MAGAT_ prefix.  All twenty-one (round 5: the A/B switches of kernel forms that lost their measurements are gone
 * with those forms; round 6: + CSR_FUSED, LAT_AGENTS, GAT_WIDE_FROM; then CHAIN_TILE16; csrc/options.hip holds the table):
 *   CHAIN_TILE16 (2) one-launch chain kernel: layer3.conv2 on 16-row tiles (v_mfma_f32_16x16x32_f16) - 0 never, 1 always, 2 from
 *                    10 240 agents (magat_encoder_desc.form_agents when set); needs off[31]; NOT bit-identical to the 32-row form
 *   LAT_AGENTS (512) largest agent count (magat_encoder_desc.form_agents when set) whose encoder runs ONE AGENT PER WORKGROUP
 *                    (csrc/block_lat.hip: layer1.conv2 .. layer3, pool, head and compressMLP in one launch; the batch-1 step of the
 *                    reference's inference loop); results bit-identical to the eight-agent-group kernels; 0 = never
 *   RANGE_GUARD (1)  split-arithmetic range guard (encoder and graph layer): see magat_encoder_read_status
 *   CONV_SPLIT  (7)  bit l: BasicBlock l+1 on the f16x3 split kernels; 0 = every convolution on the fp32 MFMA kernel (strict float32)
 *   CONV_PCHAIN (1), CONV_TM (2)  activation layout / tile height of the f16x3 split GEMMs (f16 plane granules against
 *                    float32 tiles, 256- against 128-agent tiles)
 *   L1_FUSED    (2)  stem + layer1.conv1 as one kernel: 2 = eight-agent groups (11 x 11 maps), 1 = row bands, 0 = two launches
 *   BLOCK_FUSED (2)  BasicBlock chain with the 6 x 6 maps of eight agents in LDS: 2 = layer1.conv2 -> layer2 -> layer3 -> pool as
 *                    ONE launch, 1 = two launches, 0 = one launch per convolution
 *   HEAD_F16    (1)  encoder head (and compressMLP) as f16x3 split products when its input is the chain kernel's pooled map
 *   HEAD_COMPRESS (1) compressMLP in the head GEMM's epilogue (one launch, bit-identical; from 32 768 agents on)
 *   HEAD_SPLITK (5120) largest agent count whose encoder head sums per-cell partials; decided on magat_encoder_desc.form_agents
 *                    when a shard sets it (bit-exact resharding with default options)
 *   CONV_BNFILL (256) f16x3 GEMMs with few agent tiles (the head at a few thousand agents) narrow their 128-column tile to 64 / 32
 *                    until the launch has this many workgroups; results are bit-identical for every value
 *   ENC_CHUNK (65536), GAT_CHUNK_MB (2048)  workspace bounds: agents per encoder pass, size of the two-launch graph layer's maps
 *   GAT_MFMA    (1)  graph layer with G = F = 128, N <= 102, K = 2 | 3, A_opt == NULL as ONE launch of matrix-core products
 *                    (maps, scores, softmax, hops; csrc/gat_mfma.hip; G = F in {32, 64}: N <= 32 csrc/gat_small.hip, 33 <= N <= 128
 *                    csrc/gat_mid.hip - round 6; G = F = 128 from GAT_WIDE_FROM (103, the lowest) to 128 agents: csrc/gat_mid.hip
 *                    with the X fragments in registers - between 102 and a larger value the two-launch form / CSR kernels); 0 = maps
 *                    GEMM + graph kernel;  GAT_SPLIT (1) that GEMM on the split kernels;  GAT_PACK (1) four instances per pass
 *                    at N <= 32 once the batch fills the chip (bit-identical)
 *   CSR_TILED   (3)  CSR path (N > 128 / bf16 storage): LDS-tiled score / hop kernels;  SKINNY (1) the action head as streamed
 *                    dot products
 *   CSR_FUSED   (1)  bf16-storage CSR layer, KeyQuery, K = 2, G = F = 128, concat, P in {1, 2, 4} (BASELINE config 5): the maps on
 *                    the matrix cores INSIDE the score / hop kernels, hop on the node features (csrc/gat_csr_fused.hip: no maps
 *                    GEMM, no Z in memory); 0 = maps GEMM + the CSR_TILED kernels
 * Returns MAGAT_ERR_UNSUPPORTED for an unknown name. */
int magat_set_option(const char* name, int value);
int magat_get_option(const char* name, int* value);
int magat_reset_option(const char* name);   /* back to the value the process started with: MAGAT_<NAME> from the environment if it
                                                was set, else the built-in default (ABI 6; was: always the built-in default) */

/* ------------------------------------------------------------------------------------------
 * GAT layer: GraphFilterBatchAttentional.forward  (utils/graphUtils/graphML.py:4636-4671)
 *   = graphAttentionLSIGFBatch_{KeyQuery,modified} (graphML.py:1724-1827)
 *   + learnAttentionGSOBatch{_KeyQuery,}           (graphML.py:1180-1286, 713-823)
 *   + ReLU / head concat or head mean              (graphML.py:4654-4667)
 *
 * X  [B,N,G]  row-major node features (= reference x (B,G,N) transposed; it is what
 *             compressMLP produces before the reference's permute, …bottleneck.py:302-306)
 * S  [B,N,N]  GSO exactly as handed to addGSO (float32, or float64 when s_is_f64 != 0);
 *             only |S| > 1e-9 is used (graphML.py:1274-1276).  NaN entries are non-edges.
 * weight      KeyQuery: (P,1,G,G); GAT_modified: (P,1,F,G)          GFL.0.weight
 * weight_bias (P,1,F)   used by GAT_modified only                   GFL.0.weight_bias
 * mixer       (P,1,2F)  used by GAT_modified only                   GFL.0.mixer
 * taps        (P,F,1,K,G)                                           GFL.0.filterWeight
 * bias        (F) or NULL                                           GFL.0.bias
 * Y  concat: [B,N,P*F] with feature index p*F+f (graphML.py:4657-4662); mean: [B,N,F]
 *    (= reference output (B,PF|F,N) transposed, i.e. already in the (B*N, features) layout
 *    actionsMLP consumes, …bottleneck.py:331).  ldy = row stride of Y in floats (>= width),
 *    so Y may be a column block of a wider skip-concat buffer.
 * Alignment (every graph-layer entry point: magat_gat_forward_{packed,planned,tail,dense}_f32, magat_gat_forward_csr_{f32,bf16},
 *    magat_gat_forward_csc_{f32,bf16,bf16_f32out}, magat_gnn_forward_csr_f32, magat_gnn_forward_dense_f32): X must start on a 16-byte boundary - otherwise
 *    MAGAT_ERR_UNSUPPORTED before anything is launched (its rows are read in 16-byte pieces).  ldy must be a multiple of 4
 *    (MAGAT_ERR_BAD_SHAPE).  Y may start anywhere a float (bf16: an element) may, a column block at an odd column offset
 *    included - with two exceptions, each answered with MAGAT_ERR_UNSUPPORTED before anything is launched:
 *    (1) dense entries, 128 features on 106 .. 128 agents (beyond the two-launch form's tiles, only the one-launch kernel
 *        covers them): Y on a 16-byte boundary (the *_csr_* / *_csc_* entry points take that shape at any Y);
 *    (2) magat_gat_forward_csc_bf16 and magat_gat_forward_csc_bf16_f32out in their fused form (option CSR_FUSED, on by
 *        default; KeyQuery, K = 2, G = F = 128, concat, P in {1, 2, 4}): Y and bias on a 16-byte boundary, and ldy a multiple
 *        of 8 for bf16 rows (4 for float32 rows).  magat_gat_forward_csr_bf16 takes that shape at any Y.
 *    Nothing outside the result block of Y is written.
 * A_opt [B,P,N,N] attention (aij of graphML.py:4650) or NULL (not materialised).
 * Supported: G,F in {16,32,64,128,256}, 1 <= N <= 128 (dense mask path), K >= 1, P >= 1.
 */
int magat_gat_dense_supported(int N, int G, int F); /* 1: dense-GSO kernel covers it; 0: use the *_csr_* entry point */
/* 1 when magat_gat_forward_{packed,planned}_f32 with A_opt == NULL runs this shape as ONE launch of matrix-core products
 * (gat_mfma.hip; profiling tag MAGAT_TAG_GAT_LAYER) under the current options, 0 when it takes the two-launch form (maps GEMM
 * + graph kernel).  Same results either way; tests use it to assert which kernel produced the numbers they compared. */
int magat_gat_one_launch_supported(int N, int G, int F, int K, int mode, int concat);
size_t magat_gat_packed_floats(int G, int F, int K, int P, int mode);
int magat_gat_pack_weights(const float* weight, const float* weight_bias, const float* mixer,
                           const float* taps, float* packed, int G, int F, int K, int P, int mode,
                           void* stream);
size_t magat_gat_workspace_bytes(int B, int N, int G, int F, int K, int P, int mode, int concat);
/* Range guard of the layer's per-agent maps (the f16x3 GEMM X @ [W_p | H_pk]^T; same scheme as magat_encoder_read_status):
 * the first 256 bytes of the dense AND the csr_f32 workspaces are the status block, int32 [0] = 1 when the last forward had
 * an |X| > 65504 and the maps were recomputed on the float32 MFMA kernel in the same stream, [1] = number of such re-runs
 * since the caller zeroed the block.  Synchronises `stream`. */
int magat_gat_read_status(const void* workspace, int32_t status_host[2], void* stream);
int magat_gat_forward_packed_f32(const float* X, const void* S, int s_is_f64, const float* packed,
                                 const float* bias, float* Y, int ldy, float* A_opt, void* workspace,
                                 size_t workspace_bytes, int B, int N, int G, int F, int K, int P,
                                 int mode, int concat, void* stream);

/* (ABI 7) The optional GSO plan of ABI 2-6 (magat_gat_gso_plan / magat_gat_gso_plan_bytes: edge masks + a balanced instance
 * walk made at addGSO time) is gone: opt-in, measured slower, never the default.  magat_gat_forward_planned_f32 keeps its
 * signature for existing bindings; `plan` must be NULL (anything else: MAGAT_ERR_UNSUPPORTED) - it then IS
 * magat_gat_forward_packed_f32. */
int magat_gat_forward_planned_f32(const float* X, const void* S, int s_is_f64, const float* packed,
                                 const float* bias, float* Y, int ldy, float* A_opt, void* workspace,
                                 size_t workspace_bytes, int B, int N, int G, int F, int K, int P,
                                 int mode, int concat, const void* plan, void* stream);
/* convenience: pack (into the tail of workspace) + forward; workspace must hold
 * magat_gat_workspace_bytes(...) + 4*magat_gat_packed_floats(...) bytes. */
int magat_gat_forward_dense_f32(const float* X, const void* S, int s_is_f64, const float* weight,
                                const float* weight_bias, const float* mixer, const float* taps,
                                const float* bias, float* Y, int ldy, float* A_opt, void* workspace,
                                size_t workspace_bytes, int B, int N, int G, int F, int K, int P,
                                int mode, int concat, void* stream);

/* Sparse / large-graph form of the same layer (BASELINE config 5: N = 1000 agents, comm-radius graph).  The GSO is
 * given as its edge structure: rowptr [B*(N+1)] ABSOLUTE offsets into colidx (rowptr[b*(N+1)+N] == rowptr[(b+1)*(N+1)]),
 * colidx[e] = j of the e-th edge i -> j, i.e. exactly the entries with |S[b,i,j]| > 1e-9 (graphML.py:1274-1276),
 * ascending j inside a row.  att_opt [P][nnz] receives the attention values in CSR order (or NULL).
 * Any N (<= 8190), G == F in {16,32,64,128,256}.  Gathers feature rows from global memory (L2) instead of LDS. */
size_t magat_gat_csr_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode, int concat);
int magat_gat_forward_csr_f32(const float* X, const int* rowptr, const int* colidx, long long nnz, const float* packed,
                              const float* bias, float* Y, int ldy, float* att_opt, void* workspace,
                              size_t workspace_bytes, int B, int N, int G, int F, int K, int P, int mode, int concat,
                              void* stream);
/* GraphFilterBatch.forward (graphML.py:5670-5689 -> BatchLSIGF :5485-5579), the non-attentional GNN baseline of the paper
 * (SURVEY.md 8(f) row 2):  Y[n,f] = bias[f] + sum_k sum_g (x S^k)[g,n] h[f,0,k,g]  evaluated in the same Horner form on
 * the CSR kernels, the edge weights being the GSO values vals[e] = float(S[b,i,j]) in CSR order (edges = entries with
 * float(S) != 0: magat_gso_row_degrees / magat_gso_fill_csr with rule 2).  packed = magat_gat_pack_weights(weight = NULL,
 * NULL, NULL, taps = weight (F,1,K,G), ..., P = 1, MAGAT_MODE_GNN).  F in {16,32,64,128,256}, G % 4 == 0, any N <= 8190.
 * Workspace: magat_gat_csr_workspace_bytes(B, N, nnz, G, F, K, 1, MAGAT_MODE_GNN, 1). */
int magat_gnn_forward_csr_f32(const float* X, const int* rowptr, const int* colidx, const float* vals, long long nnz,
                              const float* packed, const float* bias, float* Y, int ldy, void* workspace,
                              size_t workspace_bytes, int B, int N, int G, int F, int K, void* stream);
/* GraphFilterBatch.forward on a DENSE GSO in one launch (gnn_dense.hip; profiling tag MAGAT_TAG_GNN_DENSE, form
 * MAGAT_FORM_GNN_DENSE): the graph layer of the bottleneck GNN planners, with their ReLU fused (relu != 0).
 *   Y[b,n,f] = act(bias[f] + sum_k sum_g (x S^k)[g,n] h[f,0,k,g])   (graphML.py:5485-5579; x @ S.float() as :5562)
 * X [B*Nin][ldx] float32 rows (the encoder's compressMLP output).  S [B][N][N] float32 or float64 (s_is_f64), exactly as
 * addGSO left it; a float64 entry is rounded to float32 to nearest even.  S is a plain dense operand: every entry is
 * multiplied in, zeros included, so a NaN entry propagates as through the reference's matmul (no edge rule, no scrub).
 * weight: the RAW taps (F,1,K,G) float32 contiguous (no packing, no workspace); bias [F] or NULL.
 * Nin <= N agents: rows Nin..N-1 of the signal are the reference's zero padding (graphML.py:5675-5680) and only the Nin
 * rows of each instance are written (Y [B*Nin][ldy]).  Arithmetic: true float32 FMA chains in the Horner form on F-wide rows,
 * acc = U_{K-1}; acc = S^T acc + U_k (U_k = X H_k^T), one workgroup per (instance, 16 | 32-column slice of F).
 * Supported: 1 <= N <= 128, G, F in {16, 32, 64, 128} (G != F allowed), 1 <= K <= 8; any other shape returns
 * MAGAT_ERR_UNSUPPORTED before anything is launched (the caller then takes magat_gnn_forward_csr_f32). */
int magat_gnn_forward_dense_f32(const float* X, int ldx, const void* S, int s_is_f64, const float* weight, const float* bias,
                                float* Y, int ldy, int B, int N, int Nin, int G, int F, int K, int relu, void* stream);
/* 1: a graph of N agents with these widths and tap count is one magat_gnn_forward_dense_f32 serves (the "Supported" line above,
 * the test that entry itself makes first); 0: it answers MAGAT_ERR_UNSUPPORTED.  Additive behind ABI 9. */
int magat_gnn_dense_supported(int N, int G, int F, int K);
/* bf16-STORAGE variant (BASELINE config 5: "1000 agents, CSR, bf16"; SURVEY.md 8(b) `..._csr_{f32,bf16}`): X, the hoisted
 * maps Z, the hop intermediates and Y are bf16 in HBM (raw uint16 bit patterns, RNE), all arithmetic accumulates in
 * fp32 (bf16 MFMA for the maps GEMM with the RNE-bf16 plane of the packed weights; fp32 scores / softmax / gathers),
 * attention values stay fp32.  Same packed weights as the f32 entry point.  Needs G % 32 == 0.  ldy in elements. */
size_t magat_gat_csr_bf16_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode, int concat);
int magat_gat_forward_csr_bf16(const uint16_t* X, const int* rowptr, const int* colidx, long long nnz,
                               const float* packed, const float* bias, uint16_t* Y, int ldy, float* att_opt,
                               void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int P,
                               int mode, int concat, void* stream);
/* Row-block casts around the bf16-storage layer: src [M][ld_src] -> dst [M][ld_dst], `width` columns (multiples of 4);
 * to_bf16 != 0: float32 -> bf16 bits (RNE), else bf16 bits -> float32. */
int magat_cast_rows(const void* src, void* dst, int to_bf16, long long M, int width, int ld_src, int ld_dst, void* stream);
/* Training support (caller: loss.backward() at agents/decentralplannerlocal_OnlineExpert_GAT.py:564).
 * Forward that keeps what the backward needs: Ypre [M][P*F] = per-head filter outputs + bias BEFORE ReLU / head merge
 * (the caller's autograd owns those), att [P][nnz] (CSR order), Z [M][NC], T [(K-2)][M][P*F] (intermediate hop
 * states, NULL if K <= 2) and the CSC view (cscptr [B*(N+1)], cscsrc/cscpos/csctmp [nnz]).
 * Backward of the graph part: dZ [M][NC] (gradient wrt every column of Z) and dXd [M][G] (direct score term of dX);
 * the caller finishes with two plain GEMMs  dX = dXd + dZ @ Bt,  dBt = dZ^T @ X.  datt [P][nnz] is scratch.
 * Both answer before anything is launched, in this order: a NULL among the pointers the shape uses (colidx may be NULL when
 * nnz == 0, T when K <= 2, bias always) MAGAT_ERR_NULL; B, N, K, P <= 0 or nnz < 0 MAGAT_ERR_BAD_SHAPE; a mode that is not one
 * of the three attention modes, G != F, a width outside {16,32,64,128,256} and (forward: it transposes the GSO) N > 8190
 * MAGAT_ERR_UNSUPPORTED; more than 2^31 - 1 rows (forward) or workgroups in the largest launch MAGAT_ERR_BAD_SHAPE. */
int magat_gat_train_forward_f32(const float* X, const int* rowptr, const int* colidx, long long nnz, const float* packed,
                                const float* bias, float* Ypre, float* att, float* Z, float* T, int* cscptr,
                                int* cscsrc, int* cscpos, int* csctmp, int B, int N, int G, int F, int K, int P,
                                int mode, void* stream);
int magat_gat_train_backward_f32(const float* dYpre, const float* X, const float* Z, const float* att, const float* T,
                                 const int* rowptr, const int* colidx, const int* cscptr, const int* cscsrc,
                                 const int* cscpos, long long nnz, float* dZ, float* dXd, float* datt, int B, int N,
                                 int G, int F, int K, int P, int mode, void* stream);
/* The same pair for attentionMode 'GAT_Similarity' (P = E = 1, F = G, float32): cosine scores are KeyQuery scores of normalised
 * operands, so the forward runs the KeyQuery launches behind the normalisation kernel and keeps what that kernel did, and the
 * backward runs the KeyQuery backward on the normalised rows and pushes the two score gradients back through the normalisation.
 * `packed`: KeyQuery's layout (magat_gat_pack_weights with either mode), NC = G + K*G, score columns at 0, U_k at G + k*G.
 * Forward, beyond the outputs above: Xhat [M][G] = x_m / max(|x_m|, 1e-9) and norms [2][M] = the unclamped |x_m|, then |q_m|
 * (float32 sums of squares).  AFTER THE CALL THE SCORE COLUMNS OF Z HOLD q^_m = q_m / max(|q_m|, 1e-9), NOT q_m.
 * Backward: per row and v in {x, q}, c = max(n, 1e-9):  dv = (1/c) (dv^ - (dv^ . v^) u),  u = v^ (c/n) if n > 0 else 0  - for a
 * clamped row u is still the true unit vector (what torch's cosine_similarity differentiates to), for a zero row dv = dv^ 1e9.
 * dXd and the score columns of dZ leave the call as gradients wrt x and q; the caller's two GEMMs are the KeyQuery ones.
 * Refusals before anything is launched, in the order and with the codes of the pair above: NULL pointers (Xhat and norms too),
 * B, N, K <= 0 or nnz < 0, then G outside {16,32,64,128,256} and N > 8190 MAGAT_ERR_UNSUPPORTED, then more than 2^31 - 1 rows or
 * workgroups MAGAT_ERR_BAD_SHAPE.  The pair above keeps answering MAGAT_ERR_UNSUPPORTED for MAGAT_MODE_SIMILARITY.  Launch tags:
 * gat_maps_gemm, gat_prepare (both normalisation kernels), gat_graph; the forward counts in a form counter of its own (25,
 * numbered in the library: MAGAT_FORMS below stays what ABI 9 was built against). */
int magat_gat_train_forward_cos_f32(const float* X, const int* rowptr, const int* colidx, long long nnz, const float* packed,
                                    const float* bias, float* Ypre, float* att, float* Z, float* T, float* Xhat, float* norms,
                                    int* cscptr, int* cscsrc, int* cscpos, int* csctmp, int B, int N, int G, int K,
                                    void* stream);
int magat_gat_train_backward_cos_f32(const float* dYpre, const float* Xhat, const float* Z, const float* att, const float* T,
                                     const float* norms, const int* rowptr, const int* colidx, const int* cscptr,
                                     const int* cscsrc, const int* cscpos, long long nnz, float* dZ, float* dXd, float* datt,
                                     int B, int N, int G, int K, void* stream);

/* Backward of the non-attentional graph filter (GraphFilterBatch / BatchLSIGF, graphML.py:5485-5700).  The layer is linear in
 * x and in the taps:  Y = b + sum_k A^k X H_k^T  (A = row operator of "x @ S"), so  dU_k = (A^T)^k dY  is the forward hop
 * run over the CSR rows of S.  dY [M][F] -> dZ [M][K*F], slice k = dU_k.  The caller finishes with two plain GEMMs:
 * dX = dZ @ Bt (Bt [K*F][G], row k*F+f = weight[f,0,k,:]),  dweight[f,0,k,:] = (dZ^T X)[k*F+f],  dbias = column sums of dY.
 * rowptr / colidx / vals: the CSR arrays magat_gnn_forward_csr_f32 takes.  Answers before anything is launched: NULL pointers
 * (colidx / vals may be NULL when nnz == 0 or K == 1), then sizes <= 0, then the width, then a hop grid past 2^31 - 1. */
int magat_gnn_backward_csr_f32(const float* dY, const int* rowptr, const int* colidx, const float* vals, long long nnz,
                               float* dZ, int B, int N, int F, int K, void* stream);

/* ---- Batched on-device simulator front-end: the two per-step host loops in front of the model.
 * magat_sim_gso: multiRobotSimNew.computeAdjacencyMatrix, fixed-radius branch (utils/new_simulator.py:783-804, called by
 *   getGSO :301-321): pos [B][N][2] int32 (row, col) -> S [B][N][N] float32|float64,  W = (euclidean distance < R) with zero
 *   diagonal, optional D^-1/2 W D^-1/2 (config.symmetric_norm), then W / lambda_max(W) when `normalize` (an edgeless
 *   instance stays zero).  Edge structure is bit-exact; lambda_max (-> lambda_out [B], may be NULL) comes from Lanczos +
 *   Sturm bisection in float64 (the reference: numpy.linalg.eigvalsh on the host), values agree to ~1e-12 relative: the walk
 *   takes up to N steps, until the largest Ritz value stands still.  N <= 2048 (otherwise MAGAT_ERR_UNSUPPORTED, nothing is
 *   launched); up to 960 agents the rows of W sit in LDS as bit masks, above that the distance test is evaluated on the fly.
 *   magat_sim_gso_radii: the same with one radius per instance (radii [B] float64 on the device).
 * magat_sim_connect_radius: the step-0 branch of computeAdjacencyMatrix (:759-768): r = R / 1.1, then r *= 1.1 until the
 *   graph (distance < r) is connected - the radius the episode keeps.  radii_out [B] float64 (the same float64 products as
 *   the reference, bit-exact), steps_out [B] (may be NULL) = number of growth steps, negative if still disconnected after
 *   max_steps.  Connectivity is tested by reachability from agent 0 (the reference: multiplicity of the Laplacian's zero
 *   eigenvalue, graphTools.isConnected :562-589 - the same predicate).  N <= 5461.
 * magat_sim_fov_states: AgentState.toInputTensor for guidance 'Project_G' (dataloader/statetransformer_Guidance.py:
 *   88-124, 185-239): obstacle map [B or 1][H][W] uint8 (non-zero = obstacle; outside the map counts as obstacle),
 *   pos / goal [B][N][2] int32 -> x [B][N][3][FOV+2][FOV+2] float32 in {0,1}: channel 0 obstacles, 1 goal or projected
 *   goal, 2 agents (self included); bit-exact. */
int magat_sim_gso(const int32_t* pos, double comm_radius, int symmetric_norm, int normalize, void* S, int s_is_f64,
                  double* lambda_out, int B, int N, void* stream);
int magat_sim_gso_radii(const int32_t* pos, const double* radii, int symmetric_norm, int normalize, void* S, int s_is_f64,
                        double* lambda_out, int B, int N, void* stream);
int magat_sim_connect_radius(const int32_t* pos, double comm_radius, double* radii_out, int32_t* steps_out, int B, int N,
                             int max_steps, void* stream);
int magat_sim_fov_states(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal,
                         float* x, int FOV, int B, int N, void* stream);

/* magat_sim_guided_states: AgentState.toInputTensor for the A*-guided encodings (dataloader/statetransformer_Guidance.py:
 *   241-495; config.guidance = LocalG_S|SD, GlobalG_S|SD, SemiLG_S|SD), bit-exact: same arguments and output layout as
 *   magat_sim_fov_states, channel 1 = the cells of the reference's A* path (offlineExpert/a_star.py:75-189, reproduced step
 *   for step: 4-connected, moves up / left / down / right, Manhattan heuristic, pop = lexicographic minimum of (f, g, row,
 *   col), a cell is closed when pushed and keeps its first pusher as parent; no path = the start cell alone).
 *     mode MAGAT_GUIDE_LOCAL:  search inside the agent's own (FOV+2)^2 window (free border ring); channel 1 also holds the
 *       (projected) goal cell.  dynamic_obstacles = 0 ('_S'): the other agents are no obstacles AND channel 2 is all zero,
 *       as in the reference; 1 ('_SD'): agents in the window block, channel 2 as magat_sim_fov_states.
 *     mode MAGAT_GUIDE_GLOBAL: search on the whole map padded by FOV/2 obstacle cells and a free one-cell ring; the agents
 *       inside this agent's FOV block when dynamic_obstacles; a goal cell of value 1 is cleared; channel 1 = the path cells
 *       that fall into the agent's window.
 *     mode MAGAT_GUIDE_SEMI:   as GLOBAL on the map the agent has seen so far: agent_view [B][N][H+2(FOV/2)][W+2(FOV/2)]
 *       uint8, caller-owned, zero at the start of an episode, updated IN PLACE (the current FOV crop is written before the
 *       search); agents in the FOV always block (dynamic_obstacles is not read).  agent_view is NULL for the other modes.
 *   One launch, one wavefront per agent, open list / closed bits / parents in LDS (sized for every cell of the canvas: the
 *   open list cannot overflow), no workspace, no host synchronisation.  Limits, answered with MAGAT_ERR_UNSUPPORTED before
 *   anything is launched: odd FOV, 3 <= FOV <= 29; GLOBAL / SEMI: H + 2(FOV/2) + 2 <= 64 and W + 2(FOV/2) + 2 <= 64 (FOV 9:
 *   maps up to 54 x 54); LOCAL: any map.  The whole path is drawn (the reference raises IndexError beyond its
 *   max_localPath cells).  An agent whose position or goal lies outside the map (no such case in the reference) is not
 *   searched: its channel 1 holds the goal marker alone (LOCAL) or nothing.
 *   Profiling tag 26 ("sim_guided"), form counter 16 - numbered in the library, MAGAT_PROF_TAGS / MAGAT_FORMS below are
 *   unchanged. */
#define MAGAT_GUIDE_LOCAL 1
#define MAGAT_GUIDE_GLOBAL 2
#define MAGAT_GUIDE_SEMI 3
int magat_sim_guided_states(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal,
                            float* x, int FOV, int B, int N, int mode, int dynamic_obstacles, uint8_t* agent_view,
                            void* stream);
/* magat_sim_guided_states_wide: MAGAT_GUIDE_GLOBAL and MAGAT_GUIDE_SEMI on maps up to 256 x 256 (any FOV the narrow entry takes:
 *   a canvas of up to 286 x 286 cells, 266 x 266 at FOV 9), the same search step for step and the same tensors; a shape the
 *   narrow entry takes gives the same bits here.  The grid / closed board and the two parent-bit boards stay in LDS, 2 to 5
 *   64-bit words a canvas row; the open list - one 64-bit entry a cell, f << 36 | g << 18 | row << 9 | col, room for every cell
 *   of the canvas - lives in `workspace`: min(B N, 1024) workgroups of one wavefront are launched, each owns one slab of
 *   (H + 2(FOV/2) + 2) (W + 2(FOV/2) + 2) entries and walks the agents blockIdx, blockIdx + gridDim, ...
 *   magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV) = min(B N, 1024) * canvas rows * canvas columns * 8 (0 for a
 *   shape the entry refuses); 8-byte aligned; not read before it is written, nothing to zero.  Checks in the narrow entry's
 *   order and with its codes, MAGAT_GUIDE_LOCAL and H or W > 256 MAGAT_ERR_UNSUPPORTED; then workspace NULL MAGAT_ERR_NULL,
 *   too small MAGAT_ERR_UNSUPPORTED, misaligned MAGAT_ERR_WORKSPACE (magat_sim_mapf_plan_wide's codes) - nothing is launched.
 *   Same profiling tag and form counter as the narrow entry, no host synchronisation. */
size_t magat_sim_guided_states_wide_workspace_bytes(int B, int N, int H, int W, int FOV);
int magat_sim_guided_states_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal,
                                 float* x, int FOV, int B, int N, int mode, int dynamic_obstacles, uint8_t* agent_view,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* magat_sim_replayed_states[_wide]: MAGAT_GUIDE_SEMI without agent_view - the state of ANY step of a known schedule in one call
 *   (expert.py: expert_samples(replay=True); memory.py: ExpertMemory(replay=True)).  The maps are static and the SEMI search
 *   writes the map's own crop into the remembered map, so after step t that map is seen AND blocked, where `seen` is the union of
 *   the FOV x FOV windows of the agent's cells 0 .. t that lie on the map (an agent whose goal is off the map is never searched
 *   and has seen nothing) and blocked = off the map or map != 0.  Per (row, agent) the wave rebuilds `seen` as bit masks a padded
 *   row - in registers (narrow) or in the LDS of the parent bits, which the search needs only afterwards (wide) - and then runs the
 *   search, goal marker, path drawing and write-out of magat_sim_guided_states[_wide]: the same tensors as stepping the case with a
 *   carried agent_view.  pos / goal (B,N,2) are the row's current cells and goals, as there.  The history of row b is step
 *   row_step[b] of case row_case[b] (int32, clamped into the source), the cell of agent n at step s is
 *     pos_table[case][s][n]             (cases, T, N, 2) int32, magat_sim_expert_schedule's layout, T <= 1024;            or
 *     cells[case][n][s] = row << 8 | col  while s < lengths[case][n], goal[case][n] behind it - magat_sim_expert_pick's store:
 *                                       cells (cases, N, Lcap) uint16, lengths (cases, N), goal (cases, N, 2); steps up to 1023.
 *   Exactly one of the two is given (the other's pointers NULL).  Steps are loaded 64 at a time; a step that repeats the cell
 *   before it costs nothing.  Checks, before anything is launched: the operands and shape limits of the guided entry of the
 *   same width with its codes; history or row_case / row_step NULL, no source, or a store with a pointer missing
 *   MAGAT_ERR_NULL; both sources MAGAT_ERR_UNSUPPORTED; cases, T (table) or Lcap (store) <= 0 MAGAT_ERR_BAD_SHAPE; T > 1024
 *   MAGAT_ERR_UNSUPPORTED; then (wide) the workspace checks of magat_sim_guided_states_wide - the same workspace size.  One
 *   launch, profiling tag 26 ("sim_guided"), form counter 24 ("sim_replay", numbered in the library); no host synchronisation. */
typedef struct magat_sim_history_desc {
  const int32_t* row_case;    /* (B,) */
  const int32_t* row_step;    /* (B,) */
  const int32_t* pos_table;   /* (cases, T, N, 2), or NULL */
  const uint16_t* cells;      /* (cases, N, Lcap), or NULL with lengths and goal */
  const int32_t* lengths;     /* (cases, N) */
  const int32_t* goal;        /* (cases, N, 2) */
  int32_t cases, T, Lcap;
} magat_sim_history_desc;
int magat_sim_replayed_states(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal,
                              float* x, int FOV, int B, int N, const magat_sim_history_desc* history, void* stream);
int magat_sim_replayed_states_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal,
                                   float* x, int FOV, int B, int N, const magat_sim_history_desc* history, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* magat_sim_move: multiRobotSimNew.move + check_collision (utils/new_simulator.py:334-454, 471-520),
 *   batched: action key = argmax of the 5 logits (convectToActionKey_softmax :863-869; or given keys `actions_in`), proposed
 *   move (up 0, left 1, down 2, right 3, stop 4), shielding in the reference's order - out of the arena, face-to-face
 *   swap, obstacle, several agents into one cell, backward cascade - and pos += move in place.  ONE deviation: where the
 *   reference lets random.choice pick among several MOVING claimants of a cell, the lowest agent index wins (equal to
 *   the reference run with random.choice := first; a stationary claimant always wins, as in the reference).
 *   Outputs (each may be NULL): actions_out [B*N], moves_out [B][N][2] int8, reached_out [B][N] (new pos == goal),
 *   flags_out [B] bit0 out-of-arena, bit1 swap, bit2 obstacle, bit3 cell conflict, bit4 a position outside the map (that
 *   agent is left alone).  One workgroup per instance,
 *   H*W*4 + 16 N bytes of LDS <= 160 KB, N <= 65535. */
int magat_sim_move(const float* logits, const int32_t* actions_in, const uint8_t* map, int map_batched, int H, int W,
                   int32_t* pos, const int32_t* goal, int32_t* actions_out, int8_t* moves_out, uint8_t* reached_out,
                   int32_t* flags_out, int B, int N, void* stream);

/* magat_sim_step: one full multiRobotSimNew.move (utils/new_simulator.py:471-549) per instance with the episode state on
 * the device.  On top of magat_sim_move:
 *   - policy 0 = convectToActionKey_softmax (argmax), 1 = convectToActionKey_sum_multinorm, 2 = convectToActionKey_
 *     exp_multinorm (:863-883).  The multinomial draw is defined by caller-supplied uniforms [B*N] float64 in [0, 1)
 *     (e.g. torch.rand on the device, seeded): inverse CDF over the float32 weights (x / sum(x), or exp(x)) in index
 *     order, accumulated in float64 - the first k with w_0 + .. + w_k > u * sum.  torch.multinomial's own stream cannot be
 *     replayed on the device; the reference run with torch.multinomial patched to this rule gives identical keys
 *     (tests/golden/sim_episode_*.npz).  A row that torch.multinomial would reject (negative / inf / nan / zero sum)
 *     falls back to the argmax key and sets flag bit 5.
 *   - bookkeeping, all int32 / uint8 and updated in place: reach_goal [B][N] (sticky), first_move [B][N] (first step with a
 *     non-stop PROPOSED key, with the reference's own "== 0 means unset" test), end_step [B][N]; the step is skipped when
 *     every agent had arrived before the call or currentstep >= maxstep, and then end_step == 0 entries become
 *     currentstep - 1 and flowtime_out / makespan_out [B] are written (:528-547).  done_out [B] = allReachGoal (evaluated
 *     before the move, as the reference returns it).  flags_out != 0 (bits 0-3) is the reference's check_predictCollsion.
 *   - flag bit 4: an agent position outside the map (the agent is left where it is and takes no part in the step). */
typedef struct magat_sim_step_desc {
  const float* logits;       /* [B][N][5] or NULL */
  const int32_t* actions_in; /* [B][N] keys when logits is NULL */
  const uint8_t* map;        /* [B or 1][H][W] */
  int32_t map_batched, H, W, B, N;
  int32_t policy;            /* 0 argmax, 1 sum_multinorm, 2 exp_multinorm */
  const double* uniforms;    /* [B][N], policies 1 and 2 */
  int32_t* pos;              /* [B][N][2] in/out */
  const int32_t* goal;       /* [B][N][2] */
  uint8_t* reach_goal;       /* [B][N] in/out */
  int32_t* first_move;       /* [B][N] in/out */
  int32_t* end_step;         /* [B][N] in/out */
  int32_t currentstep, maxstep;
  int32_t* actions_out;      /* [B][N] or NULL */
  int8_t* moves_out;         /* [B][N][2] or NULL */
  int32_t* flags_out;        /* [B] or NULL */
  int32_t* done_out;         /* [B] or NULL */
  int32_t* flowtime_out;     /* [B] or NULL */
  int32_t* makespan_out;     /* [B] or NULL */
} magat_sim_step_desc;
int magat_sim_step(const magat_sim_step_desc* d, void* stream);

/* magat_sim_move_wide / magat_sim_step_wide: magat_sim_move / magat_sim_step, rule for rule and flag for flag, with the cell
 * grid in `workspace` instead of LDS: H, W <= 256 and N <= 4096 (otherwise MAGAT_ERR_UNSUPPORTED, nothing is launched).
 * magat_sim_move_wide_workspace_bytes(B, H, W, N) = B * H * W * 4 (0 for a shape the entries refuse), 4-byte aligned, written
 * before it is read.  workspace NULL MAGAT_ERR_NULL, too small MAGAT_ERR_UNSUPPORTED, misaligned MAGAT_ERR_WORKSPACE.  One
 * workgroup per instance, 16 N bytes of LDS. */
size_t magat_sim_move_wide_workspace_bytes(int B, int H, int W, int N);
int magat_sim_move_wide(const float* logits, const int32_t* actions_in, const uint8_t* map, int map_batched, int H, int W,
                        int32_t* pos, const int32_t* goal, int32_t* actions_out, int8_t* moves_out, uint8_t* reached_out,
                        int32_t* flags_out, int B, int N, void* workspace, size_t workspace_bytes, void* stream);
int magat_sim_step_wide(const magat_sim_step_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* The case pool (csrc/sim_pool.hip; rollout.py: EpisodePool): B slots over a queue of C cases, for the reference's validation /
 * test loop (agents/decentralplannerlocal_OnlineExpert_GAT.py:859-957).  A slot whose episode is over writes its case's result
 * row and takes the next case of the queue on the device; no entry synchronises with the host.
 * magat_sim_pool_step[_wide]: magat_sim_step[_wide] - the same kernel - with d->currentstep / d->maxstep replaced per slot by
 *   slot_step [B] / slot_maxstep [B] (d's two scalars are not read).  over [B] = 1 when the call finalised the slot's episode
 *   (every agent had arrived before the call, or slot_step >= slot_maxstep), else 0; sticky [B] |= the call's flag word when
 *   the slot moved.  A slot with slot_case [B] < 0 holds no case: over = 0, nothing else is read or written.  Checks and codes
 *   of magat_sim_step[_wide]; one of the five arrays NULL: MAGAT_ERR_NULL.
 * magat_sim_pool_turn: after a step.  A slot that is over writes row slot_case of the results - rows [MAGAT_POOL_COLUMNS][C]
 *   int32: retired, all_reach (done), num_reach, steps (slot_step), makespan, flowtime, predicted_collision (sticky bits 0-3),
 *   flag_bits (sticky) - and r_end_pos [C][N][2], r_first_move, r_end_step [C][N]; with `record`, traj_len [C] = steps -
 *   first_step + 1.  Then it is refilled: the finished slots take the cases next, next + 1, ... in ascending slot order (a
 *   slot's rank = the finished slots below it); start, goal and (map_batched) the map are copied in, reach_goal, first_move,
 *   end_step, sticky and the slot's agent_view (agent_view_bytes a slot; NULL: none) are zeroed, slot_step = first_step,
 *   slot_maxstep = q_maxstep[case], and radii [B] / r_radius [C] = the case's step-0 radius, magat_sim_connect_radius's loop
 *   and bits; a case still disconnected after radius_max_steps growth steps gets MAGAT_POOL_STATUS_DISCONNECTED in its status
 *   column.  Beyond the queue the slot goes idle: slot_case = -1, the positions stay.  A slot that is not over: with `record`
 *   traj [C][N][traj_cells] uint16, cell slot_step - first_step + 1, = row << 8 | col of its positions (cell 0 is the start,
 *   written at the refill); then slot_step += 1.  counters [4] int32: next, remaining, and one word handed from the turn's first
 *   launch (one wavefront: counts the finished slots, moves next and remaining) to its second (one workgroup per slot).
 *   init != 0: every slot counts as finished and no row is written - the first fill; the caller has set counters = {0, C} and
 *   zeroed rows.  N <= 5120; record: H, W <= 256; 1 <= B <= C.
 * magat_sim_pool_uniforms: u [B][N] float64 in [0, 1), 53 bits from two 32-bit draws of the case generator's stream keyed on
 *   (seed, slot_case, slot_step, agent): a case's uniforms do not depend on its slot or on B.  An idle slot gets 0. */
#define MAGAT_POOL_RETIRED 0
#define MAGAT_POOL_ALL_REACH 1
#define MAGAT_POOL_NUM_REACH 2
#define MAGAT_POOL_STEPS 3
#define MAGAT_POOL_MAKESPAN 4
#define MAGAT_POOL_FLOWTIME 5
#define MAGAT_POOL_PREDICTED 6
#define MAGAT_POOL_FLAG_BITS 7
#define MAGAT_POOL_STATUS 8
#define MAGAT_POOL_COLUMNS 9
#define MAGAT_POOL_STATUS_DISCONNECTED 2      /* status bit 1 */
typedef struct magat_sim_pool_desc {
  const uint8_t* q_map;        /* [C or 1][H][W] */
  const int32_t* q_start;      /* [C][N][2] */
  const int32_t* q_goal;       /* [C][N][2] */
  const int32_t* q_maxstep;    /* [C] */
  int32_t map_batched, H, W, C, B, N;
  int32_t first_step, record, traj_cells, radius_max_steps;
  double comm_radius;
  int32_t* slot_case;          /* [B] in/out */
  int32_t* slot_step;          /* [B] in/out */
  int32_t* slot_maxstep;       /* [B] */
  const int32_t* over;         /* [B] magat_sim_pool_step's */
  int32_t* sticky;             /* [B] */
  uint8_t* map;                /* [B][H][W] when map_batched, else NULL: the step reads q_map */
  int32_t* pos;                /* [B][N][2] */
  int32_t* goal;               /* [B][N][2] */
  uint8_t* reach_goal;         /* [B][N] */
  int32_t* first_move;         /* [B][N] */
  int32_t* end_step;           /* [B][N] */
  const int32_t* done;         /* [B] the step's done_out */
  const int32_t* flowtime;     /* [B] the step's flowtime_out */
  const int32_t* makespan;     /* [B] the step's makespan_out */
  double* radii;               /* [B] */
  uint8_t* agent_view;         /* [B][agent_view_bytes] or NULL */
  int64_t agent_view_bytes;
  int32_t* counters;           /* [4] */
  int32_t* rows;               /* [MAGAT_POOL_COLUMNS][C] */
  double* r_radius;            /* [C] */
  int32_t* r_end_pos;          /* [C][N][2] */
  int32_t* r_first_move;       /* [C][N] */
  int32_t* r_end_step;         /* [C][N] */
  uint16_t* traj;              /* [C][N][traj_cells] when record */
  int32_t* traj_len;           /* [C] when record */
} magat_sim_pool_desc;
int magat_sim_pool_step(const magat_sim_step_desc* d, const int32_t* slot_case, const int32_t* slot_step,
                        const int32_t* slot_maxstep, int32_t* over, int32_t* sticky, void* stream);
int magat_sim_pool_step_wide(const magat_sim_step_desc* d, const int32_t* slot_case, const int32_t* slot_step,
                             const int32_t* slot_maxstep, int32_t* over, int32_t* sticky, void* workspace,
                             size_t workspace_bytes, void* stream);
int magat_sim_pool_turn(const magat_sim_pool_desc* d, int init, void* stream);
int magat_sim_pool_uniforms(const int32_t* slot_case, const int32_t* slot_step, double* u, uint64_t seed, int B, int N,
                            void* stream);

/* Dense GSO -> everything the CSR kernels need, for N <= 1024, in ONE streaming pass over S plus one small kernel, with no
 * host synchronisation: addGSO's in-place scrub (scrub_nan / gso_mode 0|1 as magat_gso_prepare; values are written back only
 * where they change), the edge test (edge_rule: 0 |S| > 1e-9 in S's dtype, 1 GAT_origin |float(S) + I| > 1e-9, 2 float(S) != 0)
 * -> rowptr [B*(N+1)] absolute offsets, colidx (ascending j per row), cscptr [B*(N+1)], cscsrc / cscpos (per in-edge, ascending
 * source row: source and CSR position).  cap = capacity of colidx / cscsrc / cscpos in entries: entries beyond cap are
 * DROPPED (rowptr / cscptr still hold the true offsets) and *nnz_dev, the device-side edge total, tells - the caller reads it
 * (e.g. an asynchronous copy it waits for before the graph layer, by which time the per-agent CNN is already queued), and
 * re-builds with a larger capacity when nnz > cap; B*N*N can never overflow.  The forward entry points take `nnz` as the
 * stride of their per-head attention buffers and for sizing: any value >= the true count.  Workspace: magat_gso_csr_
 * workspace_bytes (bit matrix, N*N/8 bytes per instance; 0 = N too large, use the two calls below). */
size_t magat_gso_csr_workspace_bytes(int B, int N);
int magat_gso_csr_build(void* S, int s_is_f64, int scrub_nan, int gso_mode, int edge_rule, int* rowptr, int* colidx,
                        int* cscptr, int* cscsrc, int* cscpos, long long cap, long long* nnz_dev, void* workspace,
                        size_t workspace_bytes, int B, int N, void* stream);
/* The same build in two halves, for callers that order OTHER streams behind the in-place scrub only: phase 1 = the streaming
 * pass over S (scrub, bit matrix, edge totals: the only part that writes S), phase 2 = the structure kernel (reads the
 * workspace phase 1 left, same arguments), phase 0 = both.  An event recorded between the two is all a reader of S has to
 * wait for. */
int magat_gso_csr_build_phase(void* S, int s_is_f64, int scrub_nan, int gso_mode, int edge_rule, int* rowptr, int* colidx,
                              int* cscptr, int* cscsrc, int* cscpos, long long cap, long long* nnz_dev, void* workspace,
                              size_t workspace_bytes, int B, int N, int phase, void* stream);
/* The same edge structure straight from agent positions (gso_edges.hip; additive behind ABI 9), for the layers that read the GSO
 * through its edge test only - KeyQuery, GAT_modified, GAT_origin, GAT_Similarity: no (B,N,N) tensor and no eigenvalue, N <= 4096.
 * pos [B][N][2] int32 (row, col); (i, j), i != j, is an edge when the reference's float64 sqrt(dr^2 + dc^2) < r holds, evaluated
 * as the integer comparison magat_sim_gso uses (exact); r = radii[b] (device, float64) when radii is given, else comm_radius.
 * edge_rule 0: no self-loops (|S| > 1e-9 of the simulator's GSO); 1: every (i, i) added (|float(S) + I| > 1e-9).  Outputs in
 * magat_gso_csr_build's conventions, word for word: rowptr [B*(N+1)] absolute offsets, colidx ascending in j per row, cscptr /
 * cscsrc / cscpos per in-edge in ascending source row: the source and its CSR position.  The graph is symmetric: cscptr equals
 * rowptr and cscsrc equals colidx.  For N <= 1024 every array equals what magat_gso_csr_build makes of magat_sim_gso's tensor.
 * cap, *nnz_dev: that entry's capacity contract (entries at positions >= cap are dropped, rowptr / cscptr stay true, *nnz_dev is
 * the true total; a batch without an edge is legal).  Two launches, no host synchronisation, no atomics on device memory: the
 * arrays are the same on every call.  Workspace: magat_gso_edges_workspace_bytes (the bit matrix, N*N/8 bytes per instance, a
 * quarter of that for its word prefixes, and the row degrees; 0 = N > 4096 or a size <= 0), 256-byte aligned.
 * Answers before anything is launched: NULL pointers MAGAT_ERR_NULL (radii may be NULL; colidx, cscsrc and cscpos only with
 * cap == 0), then B, N <= 0, cap < 0, edge_rule outside 0 | 1, or no radii and comm_radius not > 0: MAGAT_ERR_BAD_SHAPE, then
 * N > 4096: MAGAT_ERR_UNSUPPORTED, then the workspace: MAGAT_ERR_WORKSPACE.  Profiling tag 35 ("gso_edges", one span per call;
 * 34 is unassigned), form counter 26 - numbered in the library, MAGAT_PROF_TAGS / MAGAT_FORMS below stay what ABI 9 was built
 * against. */
size_t magat_gso_edges_workspace_bytes(int B, int N);
int magat_gso_edges_build(const int32_t* pos, const double* radii /* [B] or NULL */, double comm_radius, int edge_rule /* 0 | 1 */,
                          int* rowptr, int* colidx, int* cscptr, int* cscsrc, int* cscpos, long long cap, long long* nnz_dev,
                          void* workspace, size_t workspace_bytes, int B, int N, void* stream);
/* The GSO's values on that structure (gso_edge_values.hip; additive behind ABI 9), for the layers that multiply by them -
 * GraphFilterBatch through magat_gnn_forward_csr_f32 / magat_gnn_backward_csr_f32 - without a (B,N,N) tensor, N <= 4096.
 * rowptr, colidx, nnz_dev, cap: what magat_gso_edges_build made under edge rule 0 (nnz_dev travels with the structure and must
 * not be NULL; whether an instance lies inside cap is read from rowptr, which stays true beyond it).  lambda_out [B] float64: lambda_max of W, or of
 * D^-1/2 W D^-1/2 under symmetric_norm, by magat_sim_gso's rule for more than 128 agents (Lanczos from the all-ones vector, Sturm
 * multisection of the tridiagonal matrix, up to N steps; tests/gso_lanczos_restatement.py) - 0 for an instance without an edge and
 * when normalize == 0.  vals [cap] float32: per CSR entry (i, j) the float32 of the float64 quotient 1 / div, or
 * (inv[i] * inv[j]) / div under symmetric_norm with inv[i] = sqrt(1 / degree(i)); div = lambda_max when normalize != 0, else 1.
 * Entries behind the edge count are not written.  Capacity contract: an instance whose edges do not all lie below cap is not
 * walked (lambda_out 0, no values) - the caller re-builds the structure with a larger capacity and calls again.  One launch, one
 * workgroup per instance, no host synchronisation, no atomics on device memory: the same result on every call.  Workspace:
 * magat_gso_edge_values_workspace_bytes (the tridiagonal matrix of every instance, 16 max(N, 160) + 16 bytes each - used from 4093
 * agents on, where it no longer fits the workgroup's 160 KB of LDS beside the three vectors; 0 = N > 4096
 * or a size <= 0), 256-byte aligned.  Answers before anything is launched: NULL pointers MAGAT_ERR_NULL (colidx and vals only with
 * cap == 0), then B, N <= 0 or cap < 0: MAGAT_ERR_BAD_SHAPE, then N > 4096: MAGAT_ERR_UNSUPPORTED, then the workspace:
 * MAGAT_ERR_WORKSPACE.  Booked under magat_gso_edges_build's profiling tag and form counter (one span, one count per call). */
size_t magat_gso_edge_values_workspace_bytes(int B, int N);
int magat_gso_edge_values(const int* rowptr, const int* colidx, const long long* nnz_dev, long long cap, int symmetric_norm,
                          int normalize, double* lambda_out, float* vals, void* workspace, size_t workspace_bytes, int B, int N,
                          void* stream);
/* magat_gat_forward_csr_{f32,bf16} with the CSC view from magat_gso_csr_build (no per-call transpose; workspace:
 * magat_gat_csc_workspace_bytes - the csr_* figure minus the transpose scratch, 3 * nnz ints) */
size_t magat_gat_csc_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode, int concat, int bf16);
int magat_gat_forward_csc_f32(const float* X, const int* rowptr, const int* colidx, const int* cscptr, const int* cscsrc,
                              const int* cscpos, long long nnz, const float* packed, const float* bias, float* Y, int ldy,
                              float* att_opt, void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K,
                              int P, int mode, int concat, void* stream);
int magat_gat_forward_csc_bf16(const uint16_t* X, const int* rowptr, const int* colidx, const int* cscptr,
                               const int* cscsrc, const int* cscpos, long long nnz, const float* packed, const float* bias,
                               uint16_t* Y, int ldy, float* att_opt, void* workspace, size_t workspace_bytes, int B, int N,
                               int G, int F, int K, int P, int mode, int concat, void* stream);
/* ... and with the RESULT widened to float32 by the kernel that writes it: Y [B*N][ldy] floats holding the bf16-rounded
 * values the call above stores (bit-identical after a cast), without the caller's bf16 -> float32 pass over Y */
int magat_gat_forward_csc_bf16_f32out(const uint16_t* X, const int* rowptr, const int* colidx, const int* cscptr,
                                      const int* cscsrc, const int* cscpos, long long nnz, const float* packed,
                                      const float* bias, float* Y, int ldy, float* att_opt, void* workspace,
                                      size_t workspace_bytes, int B, int N, int G, int F, int K, int P, int mode, int concat,
                                      void* stream);

/* dense GSO -> CSR in two steps (the caller prefix-sums the degrees in between): per-row edge counts, then column fill */
int magat_gso_row_degrees(const void* S, int s_is_f64, int self_loops /*edge rule: 0 |S|>1e-9, 1 GAT_origin |float(S)+I|>1e-9, 2 float(S)!=0*/, int* deg /*B*N*/, int B,
                          int N, void* stream);
int magat_gso_fill_csr(const void* S, int s_is_f64, int self_loops, const int* rowstart /*B*N*/, int* colidx, int B,
                       int N, void* stream);

/* addGSO's in-place scrub of the caller's tensor (decentralplanner_GAT_bottleneck.py:272-277):
 * scrub_nan: S[isnan(S)] = 0;  gso_mode 1 ('dist_GSO_one'): S[S>0] = 1;  2 ('full_GSO'): S = 1. */
int magat_gso_prepare(void* S, int s_is_f64, size_t count, int scrub_nan, int gso_mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense per-agent maps on fp32 MFMA (v_mfma_f32_32x32x2_f32): one "segmented-K" NT GEMM that
 * serves nn.Linear, the folded conv3x3/1x1+BN(+residual)+ReLU blocks of
 * graphs/models/resnet_pytorch.py:40-73,427-524 and the GAT layer's hoisted linear maps.
 *
 * Activations are pixel-major: in[(iy*Win+ix)][m][c], m in [0,M), row stride lda floats,
 * pixel stride in_pix_stride floats.  For output pixel (oy,ox):
 *   out[(oy*Wout+ox)][m][n] = act( bias[n] + sum_{ty,tx valid} sum_c in[iy,ix][m][c] * wt[n][(ty*kW+tx)*Cin + c]
 *                                         + sum_c in2[oy*stride2, ox*stride2][m][c] * wt[n][kH*kW*Cin + c] )
 * with iy = oy*stride - pad + ty (taps falling in the zero padding are skipped, not multiplied).
 * in2 (optional, C2 > 0) is the residual branch's 1x1 strided conv or a skip-concat source (never pooled).
 * wt is [Cout][Ktot], Ktot = kH*kW*Cin + C2.  Cin, C2, lda, lda2, ldc multiples of 4.
 */
typedef struct magat_conv_gemm_desc {
  const float* in;
  const float* in2;
  const float* wt;
  const float* bias;
  float* out;
  int64_t in_pix_stride, in2_pix_stride, out_pix_stride;
  int M;
  int Cin, lda, Hin, Win, kH, kW, stride, pad, Hout, Wout;
  int C2, lda2, W2, stride2;
  int Cout, ldc, relu;
  int tag;    /* MAGAT_TAG_* used by the optional profiling hooks (0 = untagged) */
  int pool;   /* 1: `in` is read through a 2x2 SUM-pool: logical pixel (iy,ix) of the Hin x Win map =
                 sum of physical pixels (2iy+{0,1}, 2ix+{0,1}) of a map that is pool_w pixels wide
                 (AvgPool2d(2) of resnet_pytorch.py:450 with the 1/4 folded into wt);
                 2: same addressing with MAX (nn.MaxPool2d(2) of decentralplanner_GAT_bottleneck.py:137) */
  int pool_w;
  /* Operand formats.  0 = float32.  1 = "bf16x3": every value carried as three bf16 planes x1+x2+x3 (fp32-exact
   * to 2^-24), plane p at base + p * *_plane_stride elements; with in_fmt = 1 the GEMM runs on the bf16 matrix
   * cores as six partial products (conv_gemm_bf16x6.hip) and in, in2, wt are all bf16x3 (wt planes are
   * Cout*Ktot apart).  in_fmt = 2: same kernel, but in / in2 stay float32 in memory and are split into their three
   * planes by the loader on the way into LDS (wt still bf16x3).  out_fmt = 1 makes the epilogue emit the 3-plane
   * form.  in_fmt = 3: in, in2 and wt are ONE bf16 plane each (plain bf16 GEMM, fp32 accumulate); out_fmt = 2: the
   * epilogue emits one RNE bf16 plane.  in_fmt = 4 ("f16x3"): in / in2 float32, split by the loader into TWO f16 planes
   * (22 significand bits; activations beyond +-1.3e5 would saturate); wt = [2][Cout][Ktot] f16 planes of (weight * 2^e)
   * followed by one float32 2^-e (applied to the accumulator before the bias); three f16 MFMAs per product (the
   * dropped plane-2 x plane-2 term is <= 2^-22 relative) - twice the matrix-core rate of the bf16x6 form at the same
   * measured accuracy.  Formats 1-4 need Cin, C2, Cout % 32 == 0 and no pooling. */
  int in_fmt, out_fmt;
  int64_t in_plane_stride, in2_plane_stride, out_plane_stride;
  /* Agent-tile strides (elements).  Row m of a pixel lives at  (m / 128) * tile_stride + (m % 128) * ld.
   * 0 = 128 * ld, i.e. plain row-major [M][ld] per pixel (and pixel planes *_pix_stride apart: "pixel-major").
   * The encoder uses the TILE-major form [agent tile][pixel][128][C] (pix_stride = 128*C, tile_stride =
   * npix*128*C): everything a workgroup touches is one contiguous ~0.5-2 MB run instead of <= 121 pieces a
   * multi-MB plane stride apart (channel/TLB-aliasing hazard of the plane form on large batches). */
  int64_t in_tile_stride, in2_tile_stride, out_tile_stride;
  /* Granule-major agent tiles, taken by the f16x3 direct kernel only (in_fmt 4, out_fmt 0; anything else returns
   * MAGAT_ERR_UNSUPPORTED).  in_gl covers in AND in2; tiles keep their size (ld = channel count C, 128*C*4 bytes per
   * pixel and tile).
   *   1: float32 granules - inside its 128-agent tile, element (m, c) of a pixel lives at
   *      ((c / 4) * 128 + (m % 128)) * 4 + c % 4 instead of (m % 128) * ld + c: the 16-byte channel quads of the 128
   *      agents are contiguous, which is how one MFMA fragment lane per agent loads and stores them (512-byte runs per
   *      half wave).
   *   2: f16 plane granules - the tile holds the two half-precision planes of the f16x3 form (value = plane0 + plane1;
   *      plane p at byte p*256*C of the pixel's tile), each as 16-byte granules [C/8][128 agents][8 halves]; granule
   *      (T*2 + ks)*2 + h of a 32-channel tile T holds channels 32T + 16ks + 8(i>>2) + 4h + (i&3) in slot i = 0..7, i.e.
   *      exactly what MFMA lane (agent, h) of the producing epilogue holds and what the consuming loader feeds to the
   *      matrix core as its k-step-ks operand.  The CONSUMER's weights must carry the same order: within every 32-wide
   *      K slab, column 16ks + 8h + i = the weight of channel 16ks + 8(i>>2) + 4h + (i&3) (encoder.fold_resnet packs
   *      such a copy behind each f16 weight block).  Values are split once by the producer instead of once per tap by
   *      every consumer.
   *   3: as 2, but plane 1 carries, per agent and 32-channel tile, 32 bytes OCP e4m3 of the value's f16 part h1 (granules 0, 1
   *      of the tile's plane-1 region: byte 16 h + 4 g + c = channel 8 g + 4 h + c) and 32 bytes e4m3 of (value - h1) * 2^11
   *      (granules 2, 3) instead of the f16 remainder: the "f16 + MX correction" form.  The consumer (in_gl = 3, weights =
   *      the THIRD copy of the pack: plane 1 = per row and slab [e4m3(g2 * 2^5) | e4m3(g1 * 2^-6)] in the same byte order)
   *      issues, per 32-channel slab, two f16 MFMAs for h1 g1 and one v_mfma_scale_f32_32x32x64_f8f6f4 for both correction
   *      products (K block 0 = q(h1) q(g2), block 1 = q(h2) q(g1), one power-of-two scale per block).  Same bytes as layout 2,
   *      half the matrix passes; results differ from the f16x3 form by ~3e-6 of the output scale. */
  int in_gl, out_gl;
  /* Row-major float32 output split into column tiles (f16x3 direct kernel, out_gl = 0 only): when > 0, the 128-channel tile
   * t of the output lives at out + t * out_ntile_stride (+ pixel offset) with row stride ldc, instead of at column 128 t of
   * one ldc-wide row - every workgroup then writes ONE contiguous region (the GAT maps' Z: consumed as per-instance
   * [N][128] tiles).  0 = plain rows. */
  int64_t out_ntile_stride;
  /* Per-output-pixel weights (float32 kernel only): output pixel q = oy * Wout + ox uses the weight matrix at
   * wt + q * wt_pix_stride (floats), rows ldw floats apart (ldw = 0: kH*kW*Cin + C2, the packed row).  With a 1x1 kernel over
   * a pooled map this turns one long-K GEMM into Hout*Wout independent partial products written to Hout*Wout output pixels
   * - the split-K form of the encoder head for small agent counts (encoder_f32.hip sums the partials).  0 = shared weights. */
  int64_t wt_pix_stride;
  int ldw;
  /* Range guard of the split arithmetic (ABI 2).  range_flag (device int32, may be NULL): the f16x3 / f16+MX kernels OR 1
   * into it when a value left the range their half-precision planes carry exactly (|v| > 65504 on the way into a plane
   * pair; > 448 into an fp8 correction plane) - such a value was CLAMPED and the result is not fp32-class.  run_if (device
   * int32, may be NULL): the float32 kernel (in_fmt 0) does nothing unless *run_if != 0 - the stream-ordered "re-run in
   * true fp32 if the split path clamped" that magat_encoder_forward_f32 / the GAT maps use. */
  int32_t* range_flag;
  const int32_t* run_if;
  /* Activation scale of the split arithmetic (ABI 3; see "Activation scales" at magat_encoder_calibrate_f32).  in_scale
   * (device float, may be NULL = 1; a stored 0 also means 1): a POWER OF TWO the f16x3 direct kernel multiplies its float32
   * activations with on the way into their two half-precision planes (in_fmt 4, in_gl 0), and divides its accumulators by
   * - exact, and it moves small-magnitude layers into the range where the second plane is a normal number.  acc_scale
   * (device float, may be NULL): replaces the 1 / weight-scale float stored behind an f16x3 weight block.  absmax (device
   * float, may be NULL): the float32 kernel (in_fmt 0) atomically maxes the largest |output| of the launch into it
   * (calibration passes; the word is a non-negative float compared as an integer). */
  const float* in_scale;
  const float* acc_scale;
  float* absmax;
  /* bit 0: `in` holds bf16 rows, bit 1: `in2` does (lda / lda2 in bf16 elements; width and stride multiples of 8): the graph layer's
   * bf16-storage result as the action head's input, read as it is instead of through a cast pass.  Taken by the
   * streamed-dot-product form of a layer with at most 8 outputs only (float32 1x1, option SKINNY); every other kernel returns
   * MAGAT_ERR_UNSUPPORTED. */
  int bf16_rows;
  /* A SECOND 1x1 layer computed in the epilogue of the first (ABI 6; f16x3 direct kernel only: in_fmt 4, out_fmt 0, out_gl 0,
   * float32 input, ONE output pixel, Cout == Cout2 == 128, so that a workgroup tile holds whole rows): out2 [M][ldc2] =
   * act2(out . wt2^T + bias2), with `out` still written.  wt2 = [2][Cout2][Cout] f16 planes of (weight * 2^e) followed by one
   * float32 2^-e (the in_fmt 4 weight block of that layer's own launch), in_scale2 as in_scale for that layer (NULL = 1).
   * compressMLP behind the encoder head: one launch instead of two, the 128-wide feature rows never re-read; bit for bit the
   * result of the two launches.  wt2 = NULL: no second layer.  Shapes the fused form does not take (narrowed column tiles of
   * a small batch, misaligned rows, ...) return MAGAT_ERR_UNSUPPORTED before anything is launched - the caller then
   * issues the two layers on their own. */
  const void* wt2;
  const float* bias2;
  float* out2;
  const float* in_scale2;
  int Cout2, ldc2, relu2;
  /* (ABI 7) with the second layer: its rows ALSO as RNE bfloat16, [M][ldc2_bf16] (multiple of 4; NULL = not written) - the
   * bf16-storage graph layer (BASELINE config 5) reads compressMLP's rows in that type: the cast pass between them is gone. */
  void* out2_bf16;
  int ldc2_bf16;
  int dilation;      /* (ABI 8) tap spacing of the kH x kW window (nn.Conv2d dilation; float32 kernel only): 0 | 1 = dense */
} magat_conv_gemm_desc;
int magat_conv_gemm_f32(const magat_conv_gemm_desc* desc_host, void* stream);

/* (ABI 9) GraphFilterBatchAttentional.forward (graphML.py:4636-4671) like magat_gat_forward_packed_f32 (no attention output), and -
 * when the launches the layer takes leave room for it - the skinny float32 layer that reads its rows inside the layer's LAST
 * launch: `tail` describes it (what magat_conv_gemm_f32 would be called with: a 1 x 1 product with five outputs over M = B N rows -
 * the planner's action head, graphs/models/decentralplanner_GAT_bottleneck.py:341-352).  *tail_done = 1: the tail's output is
 * written; 0: the caller runs magat_conv_gemm_f32(tail) itself (always a valid outcome: other shapes, other modes, many
 * instances).  Today the room is the predicated range-guard re-run of few instances (instances x heads <= 64, KeyQuery, 32 / 64 /
 * 128 features): the closed-loop step of one planning instance is THREE launches (encoder, graph layer, re-run + action head).
 * The tail's rows come from the same device code either way: bit-identical. */
int magat_gat_forward_tail_f32(const float* X, const void* S, int s_is_f64, const float* packed, const float* bias, float* Y,
                               int ldy, void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K, int P,
                               int mode, int concat, const magat_conv_gemm_desc* tail, int* tail_done, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training of the per-agent CNN (ABI 5; agents/decentralplannerlocal_OnlineExpert_GAT.py:556-567 trains the whole module, the
 * convolutions of resnet_pytorch.py:40-73, 427-524 are 96 % of a step's FLOPs).  The training-mode forward of a convolution and
 * its INPUT gradient are magat_conv_gemm_f32 calls (bias = NULL, relu = 0: the input gradient of a stride-1 convolution is the
 * convolution of dY with mirrored taps and swapped channel roles, wt' [Cin][(kH*kW) * Cout]; of a strided one the same over the
 * zero-stuffed dY).  The WEIGHT gradient is this entry:
 *     dW[co][ty*kW+tx][ci] = sum over output pixels (oy,ox) and agents m of dY[oy*Wout+ox][m][co] * X[iy*Win+ix][m][ci],
 *     iy = oy*stride - pad + ty (taps that fall into the padding are skipped).
 * x / dy pixel-major float32 as for magat_conv_gemm_f32 (row strides lda / ldc, pixel strides in floats); Cout % 32 == 0.
 * part: magat_conv_wgrad_workspace_floats() floats = [chunks][Cout][cin_w][kH][kW] partial sums over chunks of the contraction (agent ranges x groups of output pixels), each in
 * torch's own weight layout (cin_w <= Cin: the channels the weight tensor has - the stem's rows carry a fourth, padded
 * channel); *chunks_out (host int) = how many the caller has to add up (fixed order: deterministic gradients, no atomics). */
size_t magat_conv_wgrad_workspace_floats(int M, int Cin, int cin_w, int Cout, int kH, int kW, int npix /* Hout*Wout */);
int magat_conv_wgrad_f32(const float* x, long long x_pix_stride, int lda, const float* dy, long long dy_pix_stride, int ldc,
                         float* part, int* chunks_out, int M, int Cin, int cin_w, int Cout, int Hin, int Win, int Hout, int Wout,
                         int kH, int kW, int stride, int pad, void* stream);

/* nn.BatchNorm2d in TRAINING mode (batch statistics; resnet_pytorch.py:42-58) over pixel-major rows x[rows = pixels * agents][C]
 * (contiguous, C a power of two times 4, <= 256), ReLU fused on request:
 *   forward   y = [relu]((x - mean) * invstd * gamma + beta); save_mean / save_invstd [C] for the backward; running_mean /
 *             running_var (nullable) updated in place as nn.BatchNorm does (momentum = the exponential-average factor,
 *             unbiased variance)
 *   backward  dx, dgamma [C], dbeta [C] from dy (relu: masked by y > 0, y = the forward's output)
 * workspace: magat_bn_train_workspace_floats(rows, C) floats (0 = unsupported shape).  Deterministic (fixed summation order). */
size_t magat_bn_train_workspace_floats(long long rows, int C);
int magat_bn_train_forward_f32(const float* x, float* y, long long rows, int C, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps, int relu, float* save_mean,
                               float* save_invstd, float* workspace, void* stream);
int magat_bn_train_backward_f32(const float* x, const float* y, const float* dy, float* dx, long long rows, int C,
                                const float* gamma, const float* save_mean, const float* save_invstd, int relu, float* dgamma,
                                float* dbeta, float* workspace, void* stream);

/* Training of the action head and the loss (head_loss.hip; additive behind ABI 9): the LAST Linear of actionsMLP (width -> the
 * reference's 5 action logits), log-softmax and the loss in one pass over the head's input rows, their backward in one more.
 *   mode 0  nn.CrossEntropyLoss():  loss = mean_r(-log p[r, t_r]),  dlogits = (p - onehot) / M
 *   mode 1  the reference's graphs/losses/label_smoothing.py LabelSmoothing(5, smoothing) (LogSoftmax + KLDivLoss summed): with
 *           q = smoothing / 4 off the target and 1 - smoothing on it,  loss = sum_r sum_c q_rc (log q_rc - log p_rc)  - a SUM
 *           over the rows that carries the target's entropy term; a class with q = 0 contributes 0.  dlogits = p - q
 * magat_head_loss_forward_f32: logits [M][5] = X W^T + b (X rows ldx >= width floats apart, W [5][width], b [5] or NULL), the
 *   stable log-sum-exp (row maximum subtracted), dlogits [M][5] = d loss / d logits for grad_loss = 1, row_loss [M] (or NULL) and
 *   loss [1].  target [M] int64; one outside 0..4 is never used as an index: its row's loss and its dlogits row are NaN (and so
 *   the total), no other row changes.
 * magat_head_loss_backward_f32: with g = *grad_loss (a DEVICE scalar, read on the device)  dX [M][lddx] = g dlogits W,
 *   dW [5][width] = g dlogits^T X,  db [5] = g sum_r dlogits  (each nullable).
 * magat_action_loss_f32: the same loss and dlogits (nullable) on logits [M][ld >= 5] that something else produced.
 * Float32 arithmetic; every cross-row sum (loss, dW, db) adds per-workgroup partials in a fixed order in double: deterministic,
 * no atomics.  Two launches per call, no host synchronisation, no allocation.  workspace:
 * magat_head_loss_workspace_floats(M, width) floats, 8-byte aligned (0 = unsupported shape; magat_action_loss_f32 takes the
 * size of any supported width, e.g. 4).  Checks, before any launch: a NULL required pointer MAGAT_ERR_NULL; M or width <= 0
 * MAGAT_ERR_BAD_SHAPE; width % 4 != 0 or width > 1024, ldx / lddx / ld below its width, ldx or lddx not a multiple of 4 or X, W,
 * dX not 16-byte aligned (rows are read in 16-byte pieces), mode outside {0, 1}, smoothing outside [0, 1)
 * MAGAT_ERR_UNSUPPORTED; then a workspace that is not 8-byte aligned MAGAT_ERR_WORKSPACE.  Profiling tag 33 ("head_loss", one
 * span per call) - numbered in the library, MAGAT_PROF_TAGS below stays what ABI 9 was built against. */
size_t magat_head_loss_workspace_floats(long long M, int width);
int magat_head_loss_forward_f32(const float* X, int ldx, const float* W /*5 x width*/, const float* b /*5 or NULL*/,
                                const int64_t* target /*M*/, int mode, float smoothing, float* logits /*M x 5*/,
                                float* dlogits /*M x 5*/, float* row_loss /*M or NULL*/, float* loss /*1*/, float* workspace,
                                long long M, int width, void* stream);
int magat_head_loss_backward_f32(const float* dlogits, const float* grad_loss /*device scalar*/, const float* X, int ldx,
                                 const float* W, float* dX /*M x width or NULL*/, int lddx, float* dW /*5 x width or NULL*/,
                                 float* db /*5 or NULL*/, float* workspace, long long M, int width, void* stream);
int magat_action_loss_f32(const float* logits, int ld, const int64_t* target, int mode, float smoothing,
                          float* dlogits /*or NULL*/, float* row_loss /*or NULL*/, float* loss, float* workspace, long long M,
                          void* stream);

/* y[M,N] = act(x[M,K] @ w[N,K]^T + b)   (torch.nn.Linear; …bottleneck.py:105,160,229) */
int magat_linear_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int M,
                     int N, int K, int relu, void* stream);
/* same, with a MAGAT_TAG_* for the profiling hooks */
int magat_linear_tagged_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int M,
                            int N, int K, int relu, int tag, void* stream);

/* First encoder layer: conv3x3(3->32, pad 1, no bias)+BN+ReLU on the (M,3,H,W) NCHW state tensor
 * (resnet_pytorch.py:439-441, 495-498) -> pixel-major [H*W][M][32].  wt [32][27] BN-folded
 * (index c*9+ty*3+tx), bias [32]. */
int magat_conv_first_f32(const float* x, const float* wt, const float* bias, float* out, int M, int H,
                         int W, void* stream);
/* same, writing the TILE-major form [agent tile of 128][H*W][128][32] (out must hold ceil(M/128) full tiles) */
int magat_conv_first_tiled_f32(const float* x, const float* wt, const float* bias, float* out, int M, int H,
                               int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole per-agent encoder  ConvLayers (+Flatten+Linear for *_withMLP) -> compressMLP
 * (decentralplanner_GAT_bottleneck.py:90-166, 291-302) from a BN-folded parameter pack.
 * variant: 0 = ResNet(BasicBlock,[1,1,1]) "ResNetLarge", 1 = ResNetSlim(BasicBlock,[1,1]),
 * 2 = CNN_mode "Default": 5 x [conv3x3(bias)+BN+ReLU], MaxPool2d(2) after layers 0, 2, 4
 * (decentralplanner_GAT_bottleneck.py:118-147); pack: off[0..1] conv0, off[2+2i], off[3+2i] weight/bias of conv i+1
 * (i = 0..3), off[14] 128x128 identity (final max-pool as a pooled 1x1 GEMM), off[16..17] compressMLP.
 * The pack layout is produced by magat_pathplanning_amd.encoder.fold_resnet (documented there
 * and in DESIGN.md); offsets are passed explicitly so the ABI does not hard-code it.
 */
typedef struct magat_encoder_desc {
  int variant;     /* 0 ResNetLarge, 1 ResNetSlim, 2 CNN_mode "Default"; (ABI 8) 3 / 4: the dilated CNNs of DecentralPlannerNet
                      (config.use_dilated, use_dilated_version 1 / 2; graphs/models/decentralplanner.py:57-86, 138-162): conv-BN-ReLU
                      x 5 (x 4) with dilation 1 3 1 3 (1), MaxPool2d(2) behind layers 1 and 3; pack as for variant 2 */
  int H, W;        /* FOV+2 (11) */
  int n_feat;      /* numFeatureMap: width of `feat` (128 for *_withMLP, 1152 otherwise) */
  int n_comp;      /* bottleneckFeature G (0: skip compressMLP) */
  const float* pack; /* device pointer to the folded parameter pack */
  int64_t off[32];   /* float offsets into pack: see DESIGN.md "encoder pack".  off[31]: layer3.conv2 once more in 16-row
                        fragments (encoder.pack_block3_tile16; option CHAIN_TILE16), 0 = absent: the 32-row form at every size */
  int64_t chain_off; /* float offset of the BasicBlock chain kernel's fragment-major weights (encoder.pack_chain_weights: layer1.
                        conv2+downsample, layer2.conv1, layer2.conv2+downsample), 0 = absent -> layer-by-layer kernels (ABI 2) */
  int64_t chain3_off; /* float offset of the layer3 kernel's weights (encoder.pack_block3_weights), 0 = absent (ABI 2) */
  int64_t head16_off; /* float offset of the head weight as f16x2 planes + 2^-e (in_fmt 4), 0 = absent: the head runs as
                         f16x3 split products when its input is the layer3 kernel's pooled map (ABI 2) */
  int64_t comp16_off; /* the same for the compressMLP weight: 0 = absent (float32 MFMA); used together with head16_off (ABI 2) */
  int64_t scaled_off; /* float offset of the ACTIVATION-SCALE block (encoder.fold_activation_scales; ABI 3), 0 = absent:
                         [w0' 864 | b0' 32 | b1' 32 | bA' 32 | bB' 64 | bC' 64 | b31' 128 | b32' 128 | sA' sB' sC' s31' s32'
                          head_in feat_in pad] - the stem weights / biases of the fused chain multiplied by the power-of-two
                         scale their layer's activations are carried with, the five 1 / weight-scale floats with the scale
                         ratios folded in, and the in_scale of the head's and compressMLP's float32 loaders */
  int64_t l1frag_off; /* float offset of layer1.conv1 as fragment-major f16 planes (encoder.pack_chain_weights(rows, 32, 0):
                         [tap 9][k step 2][plane 2] 1 KB blocks + [2^-e, 0, 0, 0]; ABI 4), 0 = absent.  With it (11 x 11 maps,
                         option L1_FUSED = 2) the stem and layer1.conv1 run as the eight-agent-group kernel of block_fused.hip
                         (every stem pixel computed once, operands read straight out of LDS) instead of layer1_fused.hip */
  int form_agents;    /* ABI 6: the agent count the batch-size-dependent kernel FORMS are chosen on (the encoder head's split-K
                         form below option HEAD_SPLITK), 0 = this call's M.  A shard of a larger batch passes the GLOBAL agent
                         count here (distributed.sharded_forward does), so that every shard sums in the order the whole batch
                         would: shards then concatenate to the single-process result bit for bit whatever their size */
  void* comp_bf16;    /* ABI 7: NULL, or [M][n_comp] bfloat16 rows that receive RNE-bf16(comp) as well: written by the epilogue that
                         produces comp where it can (compressMLP in the head's launch), by a cast pass otherwise; after a range-guard
                         re-run of the encoder they are rewritten from the float32 rows (same stream, predicated on the flag) */
  int64_t headfrag_off; /* ABI 8: float offsets of the head's and compressMLP's weights as FRAGMENT-major f16 planes (encoder.
                           pack_frag_natural: the values and scale of head16 / comp16 in the order a wave fetches them), 0 = absent.  With */
  int64_t compfrag_off; /* both (ResNetLarge, 11 x 11 maps, n_feat = n_comp = 128) the few-agent encoder runs head and compressMLP in the
                           epilogue of the one-agent-per-workgroup chain kernel (block_lat.hip; option LAT_AGENTS): two launches for the
                           whole encoder, its results bit-identical to the batched forms (long-K f16x3 head, f16x3 compressMLP) */
} magat_encoder_desc;
/* Activation scales (ABI 3).  The split arithmetic carries a value as two f16 planes: exact for |v| <= 65504, but the SECOND
 * plane is a full 11-bit number only for |v| >~ 0.25 - a layer whose activations are all small (a small BatchNorm gamma: an
 * ordinary thing in a trained checkpoint) would be carried with an absolute floor of 2^-25 per value instead of fp32's
 * relative 2^-24.  ReLU networks commute with positive scaling, so every plane-forming stage of the fused encoder path carries
 * its map multiplied by a power of two chosen from the layer's measured magnitude (target: largest value ~2^10; exact, folded
 * into biases and into the 1 / weight-scale of the epilogues host-side), and the float32 loaders of the head, compressMLP
 * and the graph layer's maps multiply on load (magat_conv_gemm_desc.in_scale).  magat_encoder_calibrate_f32 measures the
 * magnitudes: ONE float32 pass (the range guard's re-run path: layer-by-layer float32 MFMA kernels) that also writes feat /
 * comp, leaving in absmax [16] (device floats, zeroed here) the largest |output| of: [0] stem, [1 + 2 l] layer(l+1).conv1,
 * [2 + 2 l] layer(l+1).conv2 + downsample (l = 0..2), [7] feat, [8] comp.  Unscaled packs (scaled_off = 0) behave as before. */
int magat_encoder_calibrate_f32(const magat_encoder_desc* desc_host, const float* x, float* feat, int ldfeat, float* comp,
                                int ldcomp, void* workspace, size_t workspace_bytes, int M, float* absmax, void* stream);
/* The first stage of the fused encoder path on its own (ABI 4; what magat_encoder_forward_f32 launches first, exported so
 * that the stage can be tested and profiled in isolation): stem conv3x3(3 -> 32)+BN+ReLU fused with layer1.conv1
 * (32 -> 32, stride 2)+BN+ReLU.  x (M,3,H,W) -> out: layer1.conv1's output, ctr: the stem output at the stride-2 pixels (the
 * input of the block's residual 1x1 branch), both as [ceil(M/128)][Ho*Wo] f16 plane-granule tiles of 32 channels
 * (in_gl = 2 above; 128*32*4 bytes per tile, the caller provides whole tiles).  form 2: groups of eight agents, every stem pixel
 * computed once (block_fused.hip stem8_kernel; 11 x 11 maps, needs desc->l1frag_off); form 1: 64-agent row bands
 * (layer1_fused.hip); form 0: what the encoder would pick (option L1_FUSED).  Uses the activation-scale block when
 * desc->scaled_off is set.  range_flag (device int32, may be NULL) is OR-ed with 1 when a value left the planes' range. */
int magat_encoder_stem_block_f32(const magat_encoder_desc* desc_host, const float* x, void* out, void* ctr, int M, int form,
                                 int32_t* range_flag, void* stream);
/* Range guard (option RANGE_GUARD, default 1).  The convolutions run as f16x3 split products (two half-precision planes per
 * value, fp32 accumulate: as accurate as the fp32 MFMA kernel while every activation stays within +-65504; the fused stem
 * carries its output 16x and needs it below 4094).  Whether a forward stayed inside is checked ON THE DEVICE: every kernel
 * that forms planes ORs a flag when it had to clamp, and the encoder then re-runs itself on the float32 MFMA kernels in
 * the same stream, predicated on that flag (two launches that return immediately when the flag is clear: the stem, and every
 * layer behind it chained in one kernel whose last workgroup also does the flag's bookkeeping), so feat / comp are fp32-class
 * either way.  The first 256 bytes of `workspace` are the status block, which the caller zeroes ONCE,
 * when it allocates the workspace (the library keeps its working flag there, clear between forwards).
 * magat_encoder_read_status copies two words to the host: status_host[0] = 1 if the LAST forward clamped and was re-run in
 * float32, status_host[1] = number of re-run forwards since the block was zeroed; it is the one call that synchronises
 * `stream`.  Cost of the guard when nothing clamps: the two launches above plus two for the graph layer's re-run, ~20 us of a
 * 2.6 ms c3 step (measured).  The block's words [0..2] and [6] are the library's, [4] is the graph layer's input scale. */
size_t magat_encoder_workspace_bytes(const magat_encoder_desc* desc_host, int M);
int magat_encoder_read_status(const void* workspace, int32_t status_host[2], void* stream);
int magat_encoder_forward_f32(const magat_encoder_desc* desc_host, const float* x /*M,3,H,W*/,
                              float* feat, int ldfeat, float* comp, int ldcomp, void* workspace,
                              size_t workspace_bytes, int M, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optional per-kernel timing (bench.py roofline leg).  When enabled every kernel the library
 * launches is bracketed by hipEvents on its launch stream; after the caller synchronises,
 * magat_profile_collect() folds them into per-tag (count, total ms).  Off by default.
 */
#define MAGAT_TAG_UNTAGGED 0
#define MAGAT_TAG_CONV_FIRST 1
#define MAGAT_TAG_BLOCK_CONV 2  /* +2*l: conv1 of BasicBlock l, +2*l+1: conv2(+downsample) of block l (l=0..2) */
#define MAGAT_TAG_HEAD 8        /* avgpool+fc(+Linear) folded conv */
#define MAGAT_TAG_COMPRESS 9
#define MAGAT_TAG_GAT_MAPS 10   /* hoisted X @ [W_p | H_pk]^T GEMM */
#define MAGAT_TAG_GAT_GRAPH 11  /* scores + softmax + hops kernel */
#define MAGAT_TAG_ACTIONS 12
#define MAGAT_TAG_HEAD_MEAN 13
#define MAGAT_TAG_GAT_PACK 14
#define MAGAT_TAG_GSO_PREPARE 15
#define MAGAT_TAG_GAT_PREPARE 16  /* edge masks + edge counts + balanced instance order for the persistent graph kernel */
#define MAGAT_TAG_RANGE_GUARD 17  /* flag reset + the predicated float32 re-run launches of the range guard (no-ops when clear) */
#define MAGAT_TAG_BLOCK_CHAIN 18  /* BasicBlock chain kernel (block_fused.hip) */
#define MAGAT_TAG_GAT_LAYER 19    /* the KeyQuery layer as one launch of matrix-core products (gat_mfma.hip) */
#define MAGAT_TAG_GSO_CSR 20      /* dense GSO -> CSR + CSC structure (magat_gso_csr_build, or the transpose inside *_csr_*) */
#define MAGAT_TAG_GAT_CAST 21     /* float32 <-> bf16 row casts around the bf16-storage graph layer */
#define MAGAT_TAG_BLOCK3 22       /* layer3 + ReLU + 2x2 pool in one launch (block_fused.hip) */
#define MAGAT_TAG_BLOCK_FULL 23   /* layer1.conv2 -> layer2 -> layer3 -> pool in one launch (block_fused.hip) */
#define MAGAT_TAG_CONV_WGRAD 24   /* weight gradient of a convolution (conv_train.hip; training) */
#define MAGAT_TAG_GNN_DENSE 25    /* GraphFilterBatch on a dense GSO in one launch (gnn_dense.hip) */
#define MAGAT_PROF_TAGS 26
int magat_gat_set_debug_buffer(long long* dev_buf); /* [grid][8] int64 phase timestamps of gat_dense_kernel; NULL = off */
int magat_profile_reserve(int spans);   /* pre-create event pairs (keeps hipEventCreate out of a timed region) */
int magat_profile_enable(int on);
int magat_profile_collect(void);
int magat_profile_read(int tag, long long* count, double* total_ms);
int magat_profile_reset(void);
/* What the device SUSTAINS on v_mfma_f32_32x32x16_f16 from registers alone (operand bits toggling), one wave per SIMD on every
 * CU, in one launch of about ms_target milliseconds: *tflops (dense f16).  The clock the chip holds under matrix load is part
 * of the figure (MI355X: 1.5-1.6 PFLOP/s against the 2.5 PFLOP/s of the 2.4 GHz peak clock).  scratch: 256 * CUs floats.
 * Synchronises the stream.  (ABI 5; bench.py's `roofline.sustained_*` keys) */
int magat_mfma_sustained_f16(double* tflops, float* scratch, int ms_target, void* stream);
/* (ABI 6) the same launch with its own clock evidence: *clock_mhz = the core clock the chip held inside it (median over the CUs
 * of core-clock cycles / 100 MHz ticks, read by the kernel itself), *per_clk = flop per clock and SIMD the rate amounts to at
 * that clock (1024 = one v_mfma_f32_32x32x16_f16 issued every 32 cycles: a matrix pipe that never idles), so that
 * sustained = clock x per_clk x SIMDs.  Either may be NULL.  scratch: 256 * CUs floats + 2 * CUs int64 behind them. */
int magat_mfma_sustained_f16_ex(double* tflops, double* clock_mhz, double* per_clk, float* scratch, int ms_target, void* stream);
/* Which FORM of a kernel the launches took since magat_form_reset (host-side counters, bumped where a launcher decides): the
 * forms that exist only at benchmark sizes are asserted by the full-size parity tests (tests/test_gpu_fullsize.py). */
#define MAGAT_FORM_HEAD_LONGK 0   /* encoder head as ONE long-K f16x3 GEMM (agents above option HEAD_SPLITK) */
#define MAGAT_FORM_HEAD_SPLITK 1  /* encoder head as per-cell partial products + sum (few agents) */
#define MAGAT_FORM_GAT_PACK 2     /* one-launch graph kernel, four instances per pass (N <= 32, batch fills the chip) */
#define MAGAT_FORM_GAT_PERSIST 3  /* one-launch graph kernel, more planning instances than workgroups (persistent walk) */
#define MAGAT_FORM_GAT_HSPLIT 4   /* one-launch graph kernel, a workgroup per (instance, head) (small batches) */
#define MAGAT_FORM_CHAIN_PERSIST 5 /* chain kernel: more 8-agent groups than workgroups (persistent group loop) */
#define MAGAT_FORM_HEAD_COMPRESS 6 /* compressMLP computed in the head GEMM's epilogue (one launch for both) */
#define MAGAT_FORM_GUARD_ONE 7    /* range guard of the encoder as one predicated launch */
#define MAGAT_FORM_CSR_FUSED 8    /* bf16-storage CSR layer with the maps inside the graph kernels (gat_csr_fused.hip) */
#define MAGAT_FORM_GAT_MID 9      /* one-launch graph layer for G = F in {32, 64} on 33 .. 128 agents (gat_mid.hip) */
#define MAGAT_FORM_CHAIN_LAT 10   /* chain kernel, latency form: one agent per workgroup (block_lat.hip; option LAT_AGENTS) */
#define MAGAT_FORM_HEAD_LAT 11    /* ... with the encoder head and compressMLP in its epilogue (ABI 8: headfrag_off / compfrag_off) */
#define MAGAT_FORM_GUARD_LAT 12   /* ... and the encoder's range guard inside the same launch (no predicated launches behind it) */
#define MAGAT_FORM_STEM_LAT 13    /* ... and the stem + layer1.conv1 in front: the whole encoder of a few-agent call is ONE launch */
#define MAGAT_FORM_ACTIONS_TAIL 14 /* the action head inside the graph layer's predicated re-run launch (magat_gat_forward_tail_f32) */
#define MAGAT_FORM_GNN_DENSE 15   /* the GNN graph filter as one dense launch (magat_gnn_forward_dense_f32) */
#define MAGAT_FORMS 16
long long magat_form_count(int id);
int magat_form_reset(void);

/* ------------------------------------------------------------------------------------------
 * Expert schedules -> training samples (sim_expert.hip; added behind ABI 9, nothing above changes).  The reference turns
 * an expert solver's schedule - one path per agent - into imitation samples on the host, per case, per step, per agent
 * (onlineExpert/DataTransformer_local_onlineExpert.py:181-223, 291-353; utils/new_simulator.py:226-277).  These three
 * entries do the integer / float64 part for C cases at once; states and GSOs come from magat_sim_fov_states /
 * magat_sim_guided_states / magat_sim_gso[_radii] on pos viewed as (C*T, N, 2).  Device pointers, stream ordered, no
 * allocation, no synchronisation; each call counts once in form "sim_expert" and is one span of its profiling tag (schedule:
 * a memset of `bad` and one kernel; radius: two kernels; stats: one kernel).
 *
 * magat_sim_expert_schedule (obtainSchedule): paths (C,N,Lmax,2) int32 (row, col), padded behind lengths (C,N); goal
 * (C,N,2); makespan (C,).  Case c has T_c = makespan[c] + 1 steps, the caller passes T = max T_c (steps at or behind T are
 * not produced).  For t < T_c: pos = path[t] (t < L) or the goal, next = path[t + 1] (t < L - 1) or the goal, target = one-hot
 * index of next - pos in the order up, left, down, right, stop.  pos (C,T,N,2) int32, target (C,T,N,5) float32, valid (C,T)
 * uint8 (rows at t >= T_c: zeros, valid 0).  A difference that is none of the five moves (the reference raises ValueError)
 * leaves that target row zero and sets bad[c] = t * N + n of the first such sample in (t, n) order; bad[c] = -1 otherwise. */
int magat_sim_expert_schedule(const int32_t* paths, const int32_t* lengths, const int32_t* goal, const int32_t* makespan,
                              int32_t* pos, float* target, uint8_t* valid, int32_t* bad, int C, int N, int Lmax, int T,
                              void* stream);
/* magat_sim_expert_radius (DataTransformer.computeAdjacencyMatrix, config.dynamic_commR): the threshold starts at comm_radius
 * itself, is carried over all steps of a case and multiplied by 1.1 (float64) until every step's graph (distance <
 * threshold) is connected; that ONE radius serves every step.  pos (C,T,N,2), valid (C,T) (invalid steps are ignored).
 * step_grow (C,T) int32 scratch / output: the multiplications step t needs on its own (0 at invalid steps, -1: still
 * disconnected after max_steps).  radii (C,) float64 = comm_radius * 1.1 * ... * 1.1 (grow_steps[c] = max_t step_grow
 * multiplications in sequence: bit-equal to the reference's chain); grow_steps[c] = -1 when a step stayed disconnected (radii[c]
 * then holds the radius at the limit).  N <= 5460 (three ints per agent in 64 KB of LDS): more is MAGAT_ERR_UNSUPPORTED. */
int magat_sim_expert_radius(const int32_t* pos, const uint8_t* valid, double comm_radius, int32_t* step_grow, double* radii,
                            int32_t* grow_steps, int C, int T, int N, int max_steps, void* stream);
/* magat_sim_expert_stats (multiRobotSimNew.getPathTarget): follows the argmax actions of target (C,T,N,5) from start (C,N,2)
 * over the valid steps.  expert_first_move / expert_end_step (C,N) int32: step + 1 of the first non-stop action / of the
 * first arrival at the goal, 0 when that never happens (the reference's "== 0" tests, reproduced); flowtimeTarget[c] = sum
 * (end - first + 1), makespanTarget[c] = max end - min first + 1; expert_pos (C,T+1,N,2) int32, row 0 = start (rows behind
 * an invalid step repeat the last position). */
int magat_sim_expert_stats(const float* target, const int32_t* start, const int32_t* goal, const uint8_t* valid,
                           int32_t* expert_first_move, int32_t* expert_end_step, int32_t* makespan_target,
                           int32_t* flowtime_target, int32_t* expert_pos, int C, int T, int N, void* stream);
/* magat_sim_expert_pick: the gather of a device-resident training set (memory.py: ExpertMemory).  The store holds `count`
 * cases of N agents as packed schedules - cells (count,N,Lcap) uint16 = row << 8 | col (maps up to 256 x 256), padded behind
 * lengths (count,N) with the path's last cell; goal (count,N,2); makespan (count,); radii (count,) float64; cum (count,) int64,
 * the inclusive prefix sums of makespan + 1; maps (count,H,W) uint8, or NULL when every case lives on one shared map.  A sample
 * is one (case, step) pair, numbered case by case: sample j belongs to the first case c with cum[c] > j (binary search), at
 * step t = j - cum[c - 1] (j itself for c = 0).  For each of the M entries of indices (M,) int64 and each agent, exactly
 * magat_sim_expert_schedule's rule: pos = cell[t] (t < L) or the goal, next = cell[t + 1] (t < L - 1) or the goal, target =
 * one-hot index of next - pos in the order up, left, down, right, stop.  Outputs: case_out, step_out (M,) int32; pos (M,N,2)
 * int32; target (M,N,5) float32; action (M,N) int64 = target.argmax(-1); goal_out (M,N,2) int32; radii_out (M,) float64; with
 * per-case maps map_out (M,H,W) uint8.  An index outside [0, cum[count - 1]) is clamped into it - the row is still a real
 * sample - and flag[0] = min(flag[0], m): the caller sets the int32 flag to INT32_MAX once and reads it when it likes.
 * Checks, in the siblings' order: NULL pointers (-5); non-positive sizes (-1); H, W > 256, M * N or M * H * W above 2^31 - 1,
 * maps and map_out not both set or both NULL (-2).  A refused call launches and counts nothing; a launched one is one kernel,
 * one count in form "sim_expert" and one span of its profiling tag. */
int magat_sim_expert_pick(const uint16_t* cells, const int32_t* lengths, const int32_t* goal, const int32_t* makespan,
                          const double* radii, const int64_t* cum, const uint8_t* maps /* NULL: shared map */,
                          const int64_t* indices, int32_t* case_out, int32_t* step_out, int32_t* pos, float* target,
                          int64_t* action, int32_t* goal_out, double* radii_out, uint8_t* map_out /* NULL iff maps is */,
                          int32_t* flag, int count, int N, int Lcap, int H, int W, int M, void* stream);

/* ------------------------------------------------------------------------------------------
 * A multi-agent path-finding expert (sim_mapf.hip; added behind ABI 9, nothing above changes): prioritized planning with an
 * exact space-time search per agent, for C cases at once - the schedules that magat_sim_expert_schedule takes.  It is NOT
 * ECBS: no bound on the flowtime, and a case can stay unsolved in a given priority order (the caller retries with another).
 * Device pointers, stream ordered, no allocation, no synchronisation; one kernel, one count in form "sim_mapf", one span of its
 * profiling tag.
 *
 * map (H,W) or (C,H,W) uint8 (non-zero: obstacle), start / goal (C,N,2) int32 (row, col), order (C,N) int32: the priority
 * order of each case, a permutation of 0..N-1 (NULL: index order).  T: the horizon, every path has at most T cells.  Agents
 * are planned one after another against the reservations of those before them: R_0 = {start}, R_{t+1} = free & ~V[t+1] &
 * (R_t | U_d shift_d(R_t & ~A_opp(d)[t+1])) (V[t]: cells held at t, A_d[t]: cells entered at t in direction d; the A term
 * forbids swaps); the agent arrives at t* = the first t with the goal in R_t behind the last t at which a planned agent holds
 * the goal, and holds it from then on; its path is traced back taking the first of up, left, down, right, stop that fits.
 * paths (C,N,T,2) int32 padded with the path's last cell, lengths (C,N) = t* + 1, makespan (C,) = max lengths - 1: the layout
 * of the expert entries above.  solved (C,) uint8; failed_agent (C,) int32: -1, or the agent at which the case stopped - no t*
 * below T, a start or goal off the map or on an obstacle, or the start / goal of an agent earlier in the order; -2: the order
 * row is no permutation.  In an unsolved case the agents planned before the failure keep their paths, the others get their
 * start cell with length 1.  workspace: magat_sim_mapf_workspace_bytes(C, T) = C * T * 5 * 64 * 8 bytes, 8-byte aligned,
 * zeroed by the call itself.  Limits: H, W <= 64, T <= 256, a workspace of that size - otherwise MAGAT_ERR_UNSUPPORTED and
 * nothing is launched. */
size_t magat_sim_mapf_workspace_bytes(int C, int T);
int magat_sim_mapf_plan(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                        const int32_t* order /* [C][N] or NULL = index order */, int32_t* paths /* [C][N][T][2] */,
                        int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* failed_agent, void* workspace,
                        size_t workspace_bytes, int C, int N, int T, void* stream);

/* ------------------------------------------------------------------------------------------
 * The wide forms of the solver above and of the case generator below (sim_mapf_wide.hip, sim_cases_wide.hip; added behind ABI 9, nothing above changes,
 * the 64 x 64 forms and their refusals included): maps up to 256 x 256, horizons up to 1024.  The same algorithms cell for
 * cell, the same output layouts, the same random streams - where both forms take a shape, they write the same bytes.  One
 * workgroup of rows(H) = 64 * ceil(H / 64) threads per case, thread = map row, words(W) = 1 (W <= 64), 2 (W <= 128) or 4 words
 * per row.  Same arguments in the same order, same order of the checks and same codes; counted in form "sim_mapf" and its
 * profiling tag like the 64 x 64 forms; stream ordered, no allocation, no synchronisation, one kernel per call.
 *
 * magat_sim_mapf_plan_wide: H, W <= 256, 1 <= T <= 1024.  workspace: magat_sim_mapf_wide_workspace_bytes(C, H, W, T) =
 * C * T * 6 * rows(H) * words(W) * 8 bytes, 8-byte aligned - per case and layer t the five reservation boards and, behind
 * them, the reachable set of the agent being planned, [case][t][V, A_up, A_left, A_down, A_right, R][row][word]; the call
 * zeroes the reservation boards itself.  (The size is 0 for a non-positive argument or H, W > 256.)
 * magat_sim_cases_generate_wide: H, W <= 256, N <= 4096 and N <= H * W; the maze bounds and first_case as below (kind and
 * everything else are documented there; the MAGAT_CASES_* values are plain ints). */
size_t magat_sim_mapf_wide_workspace_bytes(int C, int H, int W, int T);
int magat_sim_mapf_plan_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                             const int32_t* order /* [C][N] or NULL = index order */, int32_t* paths /* [C][N][T][2] */,
                             int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* failed_agent, void* workspace,
                             size_t workspace_bytes, int C, int N, int T, void* stream);
int magat_sim_cases_generate_wide(int kind, const uint8_t* map_in /* NULL unless GIVEN */, int map_batched, int H, int W,
                                  int aisles, int walk, uint64_t threshold, uint64_t seed, int64_t first_case,
                                  uint8_t* map_out /* [C][H][W] */, int32_t* start, int32_t* goal /* [C][N][2] */,
                                  int32_t* free_cells, uint8_t* valid, int C, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * Improving the solver's schedules by neighbourhood re-planning (sim_mapf_lns.hip; added behind ABI 9, nothing above changes):
 * MAPF-LNS with prioritized planning as its only building block, for C cases in one launch, one wavefront per case, no host
 * round trip per iteration.  It is still NOT ECBS and bounds nothing: the flowtime of a case never rises from one iteration to
 * the next, and a valid schedule stays valid.  Integer arithmetic only, no random numbers.  Device pointers, stream ordered,
 * no allocation, no synchronisation; one kernel, one count in form "sim_mapf_lns", one span of its own profiling tag.
 *
 * paths (C,N,T,2), lengths (C,N), makespan (C,) int32: a result of magat_sim_mapf_plan, improved IN PLACE; solved (C,) uint8
 * is read.  An agent's cell at t is paths[a][min(t, lengths[a] - 1)], its start the cell at 0, its goal the cell at
 * lengths[a] - 1.  Per case: all N paths are reserved as the solver reserves them, and d0[a], the length of a's path on empty
 * boards (the solver's search and backtrace), is computed once.  Iteration i = 0 .. iterations - 1: delay = lengths - d0; the
 * seed is the (i mod N)-th agent by (-delay, index); the neighbourhood is the seed, then - walking the seed's free path at
 * t = 0 .. d0 - 1 and the agents b in index order at each t - every b not yet in it whose cell at t is the free path's cell at
 * t, or which swaps with it (t >= 1: b's cell at t is the free path's at t - 1 and b's at t - 1 the free path's at t), while it
 * holds fewer than k; then seed + 1, seed + 2, ... (mod N) until it holds min(k, N).  Its paths are un-reserved, its agents
 * planned again in list order, each against everything reserved at that moment; the new paths replace the old ones iff every
 * agent arrived and the sum of the new lengths is STRICTLY below the old sum - else the reservations are put back.
 * makespan = max lengths - 1; flowtime_before / flowtime_after (C,) int32 = sum(lengths - 1) going in and coming out;
 * accepted (C,) int32: the iterations that were kept; status (C,) int32: 0 improved or unchanged; 1 skipped, solved == 0;
 * 2 refused - a length outside 1..T, one of the T cells of a row off the map or on an obstacle, or a step between two of them
 * that is none of the five moves.  A skipped or refused case keeps paths, lengths and makespan as they came, with both
 * flowtimes and accepted 0.  Conflicts BETWEEN the agents of an input are not looked for: the result is then unspecified, but
 * every access stays in bounds.  An agent that no accepted iteration re-planned keeps its row bit for bit.
 * workspace: magat_sim_mapf_improve_workspace_bytes(C, N, T) = C * (T * 5 * 64 * 8 + 8 * ceil(N / 2)) bytes (the boards, then
 * d0), 8-byte aligned, zeroed by the call itself.  Limits: H, W <= 64, 1 <= T <= 256, 1 <= k <= 8, 0 <= iterations <= 4096, a
 * workspace of that size - otherwise MAGAT_ERR_UNSUPPORTED and nothing is launched; NULL pointers and non-positive sizes are
 * answered first, as in magat_sim_mapf_plan. */
size_t magat_sim_mapf_improve_workspace_bytes(int C, int N, int T);
int magat_sim_mapf_improve(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved,
                           int32_t* paths /* [C][N][T][2], in place */, int32_t* lengths, int32_t* makespan,
                           int32_t* flowtime_before, int32_t* flowtime_after, int32_t* accepted, int32_t* status,
                           void* workspace, size_t workspace_bytes, int C, int N, int T, int iterations, int k, void* stream);

/* The wide form of the improver (sim_mapf_lns_wide.hip; added behind ABI 9, nothing above changes): the same rule, cell for
 * cell, on results of magat_sim_mapf_plan_wide - H, W <= 256, 1 <= T <= 1024 - with one workgroup of 64 * ceil(H / 64) threads per
 * case, thread = map row, 1, 2 or 4 64-bit words per row.  The arguments, the outputs, the order of the checks and the codes are
 * those of magat_sim_mapf_improve (NULL, non-positive sizes, then the limits: H, W > 256 or T > 1024, k outside 1..8,
 * iterations outside 0..4096, a workspace too small - MAGAT_ERR_UNSUPPORTED, nothing launched and nothing counted - then
 * MAGAT_ERR_WORKSPACE for a workspace that is not 8-byte aligned).  One launch, no synchronisation; it counts in form
 * "sim_mapf_lns" and is one span of that profiling tag, as the wide planner shares the planner's.
 * workspace: magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T) = C * (T * 6 * rows * words * 8 + 8 * ceil(N / 2)) bytes,
 * rows = 64 * ceil(H / 64), words = 1 (W <= 64), 2 (W <= 128) or 4: per case the layers in the wide planner's order
 * [t][V, A_up, A_left, A_down, A_right, R][row][word], then d0; 0 for a non-positive size or a side above 256. */
size_t magat_sim_mapf_improve_wide_workspace_bytes(int C, int H, int W, int N, int T);
int magat_sim_mapf_improve_wide(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved,
                                int32_t* paths /* [C][N][T][2], in place */, int32_t* lengths, int32_t* makespan,
                                int32_t* flowtime_before, int32_t* flowtime_after, int32_t* accepted, int32_t* status,
                                void* workspace, size_t workspace_bytes, int C, int N, int T, int iterations, int k,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * Auditing schedules (sim_mapf_audit.hip, sim_mapf_audit_wide.hip; added behind ABI 9, nothing above changes): is a schedule a
 * valid MAPF solution, where is its FIRST fault, and how far is its flowtime from the classic lower bound - for C cases in one
 * launch, nothing is modified.  Integer arithmetic only.  Device pointers, stream ordered, no allocation, no synchronisation;
 * one kernel, one count in form "sim_mapf_audit", one span of its own profiling tag.
 *
 * map (H,W) or (C,H,W) uint8 (non-zero: obstacle); paths (C,N,T,2), lengths (C,N), start / goal (C,N,2) int32: the layout of the
 * expert entries; solved (C,) uint8 or NULL.  Outputs, all int32:
 *   dist (C,N)      the shortest 4-connected distance over free cells from start[a] to goal[a], other agents ignored: 0 when they
 *                   are equal; -1 when either cell is off the map or on an obstacle, or when the goal is unreachable.
 *   flowtime_bound, makespan_bound (C,)   the sum and the maximum of the case's dist, both -1 when any dist of the case is -1.
 *                   Computed for EVERY case, skipped and faulty ones included: they depend on map, start and goal alone.  No
 *                   schedule of the case has a smaller flowtime / makespan.
 *   status (C,)     0 valid; 1 skipped (solved given and solved[c] == 0); 2 a fault was found.
 *   fault (C,4)     (kind, t, a, b) of the first fault, (0,-1,-1,-1) when there is none or the case is skipped.
 *   flowtime, makespan (C,)   the sum and the maximum of lengths - 1 for status 0, otherwise -1.
 * Stage 1, per agent: agents go in index order and the first agent with a fault decides; b = -1.  Within an agent, with
 * L = lengths[a], in this order: kind 1 - L outside 1..T, reported with t = -1, the agent's other checks are skipped; kind 2 -
 * paths[a,0] != start[a], t = 0; kind 3 - paths[a,L-1] != goal[a], t = L - 1; then for t = 0 .. T - 1 ascending, at each t in
 * this order: kind 4 - the cell is off the map or on an obstacle; kind 5 - t >= L and the cell differs from the cell at L - 1;
 * kind 6 - t > 0 and the step from t - 1 is none of the five moves.
 * Stage 2, conflicts, only when stage 1 found nothing in the case: the smallest (t, a, b) with a < b, at the same (t, a, b)
 * vertex before swap: kind 7, vertex - paths[a,t] == paths[b,t], t = 0 .. T - 1 (padding counts: an agent holds its goal);
 * kind 8, swap, t >= 1 - paths[a,t] == paths[b,t-1], paths[b,t] == paths[a,t-1] and a moved.  O(N T) per case: two cell-owner
 * grids for t - 1 and t, every agent takes atomicMin(owner[cell], a); only the cells that were set are cleared.
 * Bad input never faults the kernel: every cell is screened before it indexes anything - negative rows or columns, values
 * such as 2^30, a length of 0 or T + 1 are reported as above.
 * magat_sim_mapf_audit: one wavefront per case, lane = map row, the owner grids in LDS.  Limits: H, W <= 64, 1 <= T <= 256,
 * N <= 4096.  workspace: magat_sim_mapf_audit_workspace_bytes(C, N, T) = C * 2 * N * 4 bytes (the cell of every agent at t - 1
 * and at t), 8-byte aligned; 0 for a non-positive size, N > 4096 or T > 256.
 * magat_sim_mapf_audit_wide: one workgroup of 64 * ceil(H / 64) threads per case, thread = map row, 1, 2 or 4 words per row, the
 * owner grids in the workspace.  Limits: H, W <= 256, 1 <= T <= 1024, N <= 4096.  workspace:
 * magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T) = C * (2 * H * W + 2 * N) * 4 bytes (the two grids, then the cells),
 * 8-byte aligned, initialised by the call itself; 0 for a non-positive size, a side above 256, N > 4096 or T > 1024.
 * The checks come in the order and with the codes of magat_sim_mapf_improve: NULL pointers (solved may be NULL), non-positive
 * sizes, then the limits and a workspace too small - MAGAT_ERR_UNSUPPORTED, nothing launched and nothing counted - then
 * MAGAT_ERR_WORKSPACE for a workspace that is not 8-byte aligned. */
size_t magat_sim_mapf_audit_workspace_bytes(int C, int N, int T);
int magat_sim_mapf_audit(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved /* [C] or NULL */,
                         const int32_t* paths /* [C][N][T][2] */, const int32_t* lengths, const int32_t* start,
                         const int32_t* goal, int32_t* status, int32_t* fault /* [C][4] */, int32_t* dist /* [C][N] */,
                         int32_t* flowtime_bound, int32_t* makespan_bound, int32_t* flowtime, int32_t* makespan, void* workspace,
                         size_t workspace_bytes, int C, int N, int T, void* stream);
size_t magat_sim_mapf_audit_wide_workspace_bytes(int C, int H, int W, int N, int T);
int magat_sim_mapf_audit_wide(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved /* [C] or NULL */,
                              const int32_t* paths /* [C][N][T][2] */, const int32_t* lengths, const int32_t* start,
                              const int32_t* goal, int32_t* status, int32_t* fault /* [C][4] */, int32_t* dist /* [C][N] */,
                              int32_t* flowtime_bound, int32_t* makespan_bound, int32_t* flowtime, int32_t* makespan,
                              void* workspace, size_t workspace_bytes, int C, int N, int T, void* stream);

/* ------------------------------------------------------------------------------------------
 * An optimal expert: conflict-based search (sim_mapf_cbs.hip; added behind ABI 9, nothing above changes).  CBS (Sharon et al.
 * 2015) for C cases in one launch, one wavefront per case, every node and every search inside it: optimal in the flowtime and
 * complete up to a budget of nodes, and its open list gives a lower bound of the optimal flowtime.  Deterministic, integer
 * arithmetic only.  Device pointers, stream ordered, no allocation, no synchronisation; one kernel, one count in form
 * "sim_mapf_cbs", one span of its own profiling tag.  No focal search (that is magat_sim_mapf_ecbs, below), no pruning by an
 * incumbent, no disjoint splitting, no conflict prioritisation.
 *
 * map, start, goal, T, paths, lengths, makespan, solved: as in magat_sim_mapf_plan.  The other outputs are (C,) int32.
 * Screening, before any cell indexes anything: a start or goal off the map or on an obstacle, or a start (a goal) that an agent
 * of a lower index has too - status 3.  Then the root: every agent's FREE path, the planner's search and backtrace on empty
 * boards, agents in index order; an agent without an arrival inside T - status 2 with horizon_hit 1.  Neither makes a node.
 * Node: its parent, the agent it planned again, ONE constraint, its cost - the flowtime sum(lengths - 1) of its schedule - and
 * that agent's new path and length; node 0, the root, holds N paths.  The schedule of a node is, per agent, the path of the
 * nearest node on the chain to the root (itself first) that planned it, else the root's; the constraints of an agent are those
 * of the nodes on that chain that planned it.  A constraint is a bit of the planner's reservation boards: "agent x is not on
 * cell u at t" is bit u of V[t]; "x does not step from u in direction d, arriving at t" is bit u of A_opp(d)[t] - what the search
 * reads as a swap.  The search returns the earliest arrival behind the last t at which V[t] holds the goal, so a constraint on an
 * agent parked at its goal sends it away and back.
 * Loop: take the open node with the smallest (cost, index).  Its first conflict is the audit's stage 2 on its schedule: the
 * smallest (t, a, b), a < b, vertex before swap.  None - status 0, this schedule is the answer.  Otherwise, nodes + 2 >
 * max_nodes - status 1.  Otherwise the node counts as expanded and gets two children, for a, then for b: a vertex conflict
 * forbids the agent's cell at t (its last cell when it is parked), a swap its own step at t; the agent is searched again under
 * all its constraints, cost = the parent's - its old length + its new one.  A child whose search finds no arrival (the
 * reachable set ran empty, or t reached T - 1) keeps its slot, never enters the open list, and sets horizon_hit.  An empty open
 * list - status 2.
 *   status        0 solved, optimal among the schedules of at most T cells per path; 1 the budget ran out; 2 no schedule inside
 *                 T (or none at all); 3 screened out
 *   paths, lengths, makespan     status 0: the schedule, padded with each path's last cell; otherwise every agent's start cell
 *                 with length 1, makespan 0.  solved = (status == 0)
 *   flowtime      status 0: sum(lengths - 1); otherwise -1
 *   lower_bound   status 0: the flowtime; status 1: the cost of the node the search stopped at, the minimum over the open list;
 *                 status 2, 3: -1.  With horizon_hit == 0 no schedule of the case has a smaller flowtime; otherwise none of at
 *                 most T cells per path has.
 *   nodes         nodes created, the root included (0 for a case that got none); expanded: nodes that got their children
 *   horizon_hit   1 when a child was dropped for lack of an arrival (or the root had none), else 0
 * workspace: magat_sim_mapf_cbs_workspace_bytes(C, N, T, max_nodes) = C * 8 * (T * 5 * 64 + ceil(N * T / 4) + ceil(max_nodes *
 * T / 4) + 2 * max_nodes + ceil(N / 2) + N) bytes - per case the five constraint boards, the root's paths and the nodes' paths
 * (a cell is 16 bits, row << 8 | col), 16 bytes per node, the root's lengths, the conflict scan's two cell rows - 8-byte aligned;
 * the call zeroes and initialises what it reads; 0 for a non-positive size or one above the limits.
 * Limits: H, W <= 64, 1 <= T <= 256, N <= 4096, 1 <= max_nodes <= 4096, a workspace of that size - otherwise
 * MAGAT_ERR_UNSUPPORTED, nothing launched and nothing counted.  The checks come in the planner's order: NULL pointers, non-positive
 * sizes (max_nodes too), the limits and the workspace's size, then MAGAT_ERR_WORKSPACE for one that is not 8-byte aligned. */
size_t magat_sim_mapf_cbs_workspace_bytes(int C, int N, int T, int max_nodes);
int magat_sim_mapf_cbs(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                       int32_t* paths /* [C][N][T][2] */, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                       int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                       void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A bounded-suboptimal expert: ECBS (Barer et al. 2014), conflict-based search with a focal search on both levels
 * (sim_mapf_ecbs.hip; added behind ABI 9, nothing above changes).  C cases in one launch, one wavefront per case, as
 * magat_sim_mapf_cbs; one kernel, one count in form "sim_mapf_ecbs", one span of its own profiling tag.  Deterministic, integer
 * arithmetic only: w >= 1 comes as w_milli = round(1000 w), every comparison is made in 64 bits.
 *
 * Arguments, screening, constraints, outputs and statuses are magat_sim_mapf_cbs's, except that status 0 promises
 * 1000 * flowtime <= w_milli * lower_bound <= w_milli * optimum, not optimality.  levels = K, 1..4.
 * Boards.  HARD boards hold the searched agent's constraints, as in CBS.  SOFT boards, a second [T][5][64] set per case, hold the
 * planner's reservation (V[t] for every t < T, the parked cell included; A_d[t] at the entered cell of a real move) of every
 * OTHER agent of the schedule the search runs against; they are set before a search and cleared after it.  A step arriving at
 * t + 1 is DIRTY when its destination is in soft V[t + 1], or it is a real move from u in direction d with u in soft
 * A_opp(d)[t + 1]; a step that honours the hard and the soft boards is CLEAN.
 * Low level: K planes P^0 .. P^(K-1) of reachable cells, hard(X) the planner's step on the hard boards, clean(X) the same step on
 * (hard | soft).  P^k_0 = {start}; P^(K-1)_(t+1) = hard(P^(K-1)_t), the planner's R; P^0_(t+1) = clean(P^0_t); P^k_(t+1) =
 * clean(P^k_t) | hard(P^(k-1)_t) for 1 <= k <= K - 2: at most k dirty steps.  `last` and t* are the planner's, on plane K - 1 (no
 * arrival: as there).  The flood goes on to b = min(w_milli * t* / 1000, T - 1), integer division; the arrival is the smallest k
 * with the goal in P^k_t for a t in [t*, b], then the smallest such t.  The path has t + 1 cells, the agent's bound is t*.
 * Backtrace from (t, goal, k), candidates up, left, down, right, stop: in plane K - 1 any hard-allowed source in P^(K-1)_(t-1);
 * in a plane k below it first a source in P^k_(t-1) whose step is clean - none when the cell is in soft V[t], where it can only
 * stand by a drop - else a hard-allowed source in P^(k-1)_(t-1), and on in plane k - 1.
 * Root: the agents in index order, agent a against soft boards of agents 0 .. a - 1 and empty hard boards.
 * Node: parent, cost = sum(lengths - 1), lb = sum(t*), hc, the agent, ONE constraint, that agent's path and t*; a child's cost
 * and lb are the parent's minus the agent's old length / t* plus its new ones.  hc counts the conflicts of the node's own
 * schedule over t < max(lengths), own_t[cell] being the smallest agent on a cell at t: the agents a with own_t[cell_a(t)] < a,
 * and for t >= 1 the agents a that moved, with b = own_(t-1)[cell_a(t)] existing, b > a and cell_b(t) == cell_a(t-1).
 * Loop: LBmin = the smallest lb over the open list; among the open nodes with 1000 * cost <= w_milli * LBmin (never none) take the
 * smallest (hc, cost, index).  Its first conflict is the audit's stage 2.  None - status 0, flowtime = cost, lower_bound =
 * LBmin.  nodes + 2 > max_nodes - status 1, lower_bound = LBmin.  Otherwise two children as in CBS, each searched against soft
 * boards of the popped node's other agents; a dead child keeps its slot and sets horizon_hit.  An empty open list - status 2.
 * lower_bound bounds the optimum under CBS's horizon caveat.
 * workspace: magat_sim_mapf_ecbs_workspace_bytes(C, N, T, max_nodes, levels) = C * 8 * (T * 64 * (10 + levels) + ceil(N * T / 4)
 * + ceil(max_nodes * T / 4) + 4 * max_nodes + ceil(5 * N / 2)) bytes - per case both sets of boards, the planes, the root's and
 * the nodes' paths, 32 bytes per node, five int rows of N - 8-byte aligned; the call initialises what it reads.
 * Limits: those of magat_sim_mapf_cbs, 1 <= levels <= 4 and 1000 <= w_milli <= 2^20.  The checks come in its order: NULL
 * pointers; non-positive sizes, levels < 1 or w_milli < 1000 (MAGAT_ERR_BAD_SHAPE); the limits, levels > 4, w_milli > 2^20 and
 * the workspace's size (MAGAT_ERR_UNSUPPORTED); then its alignment.  A refused call launches and counts nothing. */
size_t magat_sim_mapf_ecbs_workspace_bytes(int C, int N, int T, int max_nodes, int levels);
int magat_sim_mapf_ecbs(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                        int32_t* paths /* [C][N][T][2] */, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                        int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                        void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, int w_milli, int levels,
                        void* stream);

/* The wide form of magat_sim_mapf_ecbs (sim_mapf_ecbs_wide.hip; added behind ABI 9, nothing above changes): the same rule, cell
 * for cell and node for node, the same arguments, outputs and statuses, on maps up to 256 x 256 with horizons up to 1024.  One
 * workgroup of rows = 64 * ceil(H / 64) threads per case, thread = map row, words = 1, 2 or 4 64-bit words per row (the smallest
 * with 64 * words >= W), as magat_sim_mapf_plan_wide; one kernel, counted in the narrow form's "sim_mapf_ecbs" and one span of its
 * profiling tag.  The cell-owner grids of the conflict scan and the conflict count live in the workspace, not in LDS.
 * workspace: magat_sim_mapf_ecbs_wide_workspace_bytes(C, H, W, N, T, max_nodes, levels) = C * 8 * (T * rows * words * (10 + levels)
 * + ceil(N * T / 4) + ceil(max_nodes * T / 4) + 4 * max_nodes + ceil(5 * N / 2) + H * W) bytes - per case both sets of boards
 * [T][5][rows][words], the planes [levels][T][rows][words], the root's and the nodes' paths, 32 bytes per node, five int rows of N
 * and the two grids of H * W ints - 8-byte aligned; the call initialises what it reads.  0 outside the limits.
 * Limits: H, W <= 256, T <= 1024, N <= 4096, max_nodes <= 4096, 1 <= levels <= 4, 1000 <= w_milli <= 2^20.  The checks come in
 * magat_sim_mapf_ecbs's order: NULL pointers; non-positive sizes, levels < 1 or w_milli < 1000 (MAGAT_ERR_BAD_SHAPE); the limits
 * and the workspace's size (MAGAT_ERR_UNSUPPORTED); then its alignment.  A refused call launches and counts nothing. */
size_t magat_sim_mapf_ecbs_wide_workspace_bytes(int C, int H, int W, int N, int T, int max_nodes, int levels);
int magat_sim_mapf_ecbs_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                             int32_t* paths /* [C][N][T][2] */, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                             int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                             void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, int w_milli, int levels,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Planning cases made on the device (sim_cases.hip; added behind ABI 9, nothing above changes): the first step of the expert
 * pipeline, the reference's offlineExpert/CasesGenerator.py - an obstacle map, its largest free component, a start and a goal
 * per agent - for C cases in one launch; its outputs are what magat_sim_mapf_plan takes.  Device pointers, stream ordered, no
 * allocation, no workspace, no synchronisation; one kernel.  It adds no profiling tag and no form of its own: as the head of
 * the same pipeline it counts once in form "sim_mapf" and is one span of that profiling tag.
 *
 * kind: MAGAT_CASES_MAZE - the reference's mapGen: `aisles` walks of `walk` steps over the even lattice (the caller computes
 * aisles = int(density * (H / 2) * (W / 2)), walk = int(complexity * 5 * (H + W))); MAGAT_CASES_UNIFORM - cell (r, c) is an
 * obstacle iff its 32-bit draw < threshold = floor(density * 2^32); MAGAT_CASES_GIVEN - map_in (H,W), or (C,H,W) when
 * map_batched, uint8, non-zero: obstacle (map_in may be NULL for the other kinds).  The kept free region is the largest
 * 4-connected free component (ties: the one holding the lowest row-major cell); every other free cell is an obstacle in
 * map_out (C,H,W) uint8 (0 / 1), free_cells (C,) = F, its size.  start / goal (C,N,2) int32 (row, col): starts are N distinct
 * cells of the region, uniform over ordered tuples, goals likewise, redrawn as a whole (at most 64 times) until goal[a] !=
 * start[a] for every agent.  valid (C,) uint8 = 1 iff F >= N + 1 and a goal tuple was accepted; otherwise start and goal are -1.
 * Random numbers: draw(seed, first_case + c, stream, index), a counter-based hash - a case depends on its
 * GLOBAL index first_case + c, not on C or its place in the batch.
 * Limits: H, W <= 64; maze: H, W >= 4, aisles <= 4096, walk <= 1024; N <= H * W; 0 <= first_case, first_case + C <= 2^32 -
 * otherwise MAGAT_ERR_UNSUPPORTED and nothing is launched (null pointers -5, non-positive sizes or an unknown kind -1). */
#define MAGAT_CASES_MAZE 0
#define MAGAT_CASES_UNIFORM 1
#define MAGAT_CASES_GIVEN 2
int magat_sim_cases_generate(int kind, const uint8_t* map_in /* NULL unless GIVEN */, int map_batched, int H, int W, int aisles,
                             int walk, uint64_t threshold, uint64_t seed, int64_t first_case, uint8_t* map_out /* [C][H][W] */,
                             int32_t* start, int32_t* goal /* [C][N][2] */, int32_t* free_cells, uint8_t* valid, int C, int N,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGAT_HIP_H */
