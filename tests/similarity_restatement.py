"""float64 numpy restatement of attentionMode 'GAT_Similarity' (the reference's GraphFilterBatchSimilarityAttentional,
graphML.py:4690-4857 with learnSimilarityAttentionGSOBatch :1449-1564 and graphSimilarityAttentionLSIGFBatch :2095-2179), one head
and one edge feature - the only configuration whose reference forward runs.  TEST INFRASTRUCTURE: the device tests compare with it
at shapes no fixture holds; test_host_similarity.py pins it on every fixture the real reference made.

    e[i][j] = (x_i / max(|x_i|, 1e-9)) . (q_j / max(|q_j|, 1e-9)),  q_j = W x_j        (no bias, no LeakyReLU)
    M       = |float32(S) + I| > 1e-9 in float32 (NaN: no edge; a diagonal -1 cancels the self-loop)
    A       = softmax_j(e M - (1 - M) 1e12) M
    z_0 = x,  z_k = z_{k-1} A,  y = relu(sum_k H_k z_k + b)
"""
import numpy as np


def similarity_mask(S):
    """S (B,N,N) | (B,1,N,N), float32 | float64 -> (B,N,N) bool."""
    S = np.asarray(S)
    S = S.reshape(S.shape[0], S.shape[-2], S.shape[-1])
    with np.errstate(invalid="ignore"):
        return np.abs(S.astype(np.float32) + np.eye(S.shape[-1], dtype=np.float32)) > np.float32(1e-9)


def similarity_layer(x, S, weight, filterWeight, bias=None):
    """x (B,G,N); S (B,N,N) | (B,1,N,N); weight (1,1,G,G); filterWeight (1,F,1,K,G); bias (F,1) | None
    -> y (B,F,N) float64 (after the ReLU; with one head concat and mean are the same), aij (B,1,1,N,N) float64."""
    x = np.asarray(x, dtype=np.float64)
    W = np.asarray(weight, dtype=np.float64)
    H = np.asarray(filterWeight, dtype=np.float64)
    assert W.shape[:2] == (1, 1) and H.shape[0] == 1 and H.shape[2] == 1, "one head, one edge feature"
    B, G, N = x.shape
    W = W.reshape(G, G)
    H = H[0, :, 0]                                              # F,K,G
    K = H.shape[1]
    M = similarity_mask(S).astype(np.float64)                   # B,N,N
    X = x.transpose(0, 2, 1)                                    # B,N,G
    Q = X @ W.T                                                 # q_j = W x_j
    Xn = X / np.maximum(np.linalg.norm(X, axis=2, keepdims=True), 1e-9)
    Qn = Q / np.maximum(np.linalg.norm(Q, axis=2, keepdims=True), 1e-9)
    e = Xn @ Qn.transpose(0, 2, 1)                              # e[b,i,j]
    t = e * M - (1.0 - M) * 1e12
    t = np.exp(t - t.max(axis=2, keepdims=True))
    A = t / t.sum(axis=2, keepdims=True) * M
    z = x
    y = np.einsum("fg,bgn->bfn", H[:, 0], z)
    for k in range(1, K):
        z = z @ A
        y = y + np.einsum("fg,bgn->bfn", H[:, k], z)
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64).reshape(1, -1, 1)
    return np.maximum(y, 0.0), A.reshape(B, 1, 1, N, N)
