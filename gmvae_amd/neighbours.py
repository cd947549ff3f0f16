"""Neighbourhood scores of a latent code on the device (include/gmvae_hip.h gmvae_knn_*; csrc/neigh.hpp): exact brute-force k nearest
neighbours with a defined total order -- distance, then index --, the rank of given candidates in that order and distance sums per
class; from them the k-NN accuracy of a code, the silhouette of a labelling on it, the trustworthiness and continuity of an
embedding, and next to them NMI and ARI of two labellings.  O(N^2), memory O(rows * N).  Model independent: codes are any fp32
[N, L] device tensor.  The statement is tests/neigh_ref.py.  Everything stays on the device; nothing synchronises with the host."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

MAX_NR, MAX_L, MAX_K, MAX_C = 1 << 24, 4096, 256, 256      # the library's gate (include/gmvae_hip.h)
D2_CHUNK_BYTES = 256 << 20      # a call's chunk of distance rows is at most this large unless `rows` says otherwise


def workspace_bytes(Nq, Nr, Lz, k=1, n_labels=1):
    b = C.c_uint64()
    L.check(L.lib.gmvae_knn_workspace_bytes(int(Nq), int(Nr), int(Lz), int(k), int(n_labels), C.byref(b)), "gmvae_knn_workspace_bytes")
    return b.value


def default_rows(Nq, Nr):
    return max(1, min(int(Nq), D2_CHUNK_BYTES // (4 * int(Nr))))


def _codes(t, what="codes"):
    t = torch.as_tensor(t).to(L.require_gpu(), torch.float32).contiguous()
    if t.dim() != 2:
        raise ValueError(f"{what} must be [N, L]")
    return t


def _pair(queries, refs, exclude_self):
    """(q, r, self): refs None = the set against itself, self excluded unless exclude_self is False."""
    q = _codes(queries, "queries")
    r = q if refs is None else _codes(refs, "refs")
    if exclude_self is None:
        exclude_self = refs is None
    if q.shape[0] < 1 or not 1 <= r.shape[0] <= MAX_NR or not 1 <= q.shape[1] <= MAX_L:
        raise ValueError(f"queries [Nq, L] and refs [Nr, L] need Nq >= 1, 1 <= Nr <= 2^24 and 1 <= L <= {MAX_L}: got "
                         f"{tuple(q.shape)}, {tuple(r.shape)}")
    if r.shape[1] != q.shape[1]:
        raise ValueError(f"queries and refs differ in L: {q.shape[1]} and {r.shape[1]}")
    if exclude_self and q.shape[0] != r.shape[0]:
        raise ValueError(f"exclude_self: query i is reference i, so the two sets have one size: got {q.shape[0]} and {r.shape[0]}")
    return q, r, bool(exclude_self)


def _rows(rows, Nq, Nr):
    rows = default_rows(Nq, Nr) if rows is None else int(rows)
    if not 1 <= rows <= Nq:
        raise ValueError(f"rows must be in [1, {Nq}]")
    return rows


def _labels(labels, n, what="labels"):
    labels = torch.as_tensor(labels).to(L.require_gpu())
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.shape != (n,):
        raise ValueError(f"{what} must be an integer tensor [{n}]")
    return labels.to(torch.int32).contiguous()


def _check_count(v, what, hi=MAX_K):
    v = int(v)
    if not 1 <= v <= hi:
        raise ValueError(f"{what} must lie in [1, {hi}]: got {v}")
    return v


def knn(queries, refs=None, k=10, exclude_self=None, rows=None):
    """The k nearest references of every query in the order (distance, index): a dict of `idx` [Nq, k] (int32) and `d2` [Nq, k]
    (fp32, the squared distances), ascending.  refs=None: the set against itself with self excluded.  exclude_self with refs given:
    query i is reference i.  rows: queries per call (the workspace holds rows * Nr distances)."""
    q, r, ex = _pair(queries, refs, exclude_self)
    Nq, Lz = q.shape
    Nr = r.shape[0]
    k = _check_count(k, "k")
    if k > Nr - (1 if ex else 0):
        raise ValueError(f"k = {k} exceeds the {Nr - (1 if ex else 0)} references a query has")
    rows = _rows(rows, Nq, Nr)
    ws = torch.empty(workspace_bytes(rows, Nr, Lz, k), dtype=torch.uint8, device=q.device)
    idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    d2 = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    for r0 in range(0, Nq, rows):
        n = min(rows, Nq - r0)
        L.check(L.lib.gmvae_knn_search(L.ptr(q[r0:]), n, L.ptr(r), Nr, Lz, k, r0 if ex else -1, L.ptr(idx[r0:]), L.ptr(d2[r0:]),
                                       L.ptr(ws), L.current_stream()), "gmvae_knn_search")
    return {"idx": idx, "d2": d2}


def ranks(queries, refs, cand, exclude_self=False, rows=None):
    """rank [Nq, m] (int32): the number of references (self left out under exclude_self) strictly in front of cand[i, t] in query
    i's order; -1 for a candidate that is self or no reference.  ranks(knn's idx)[i, t] == t."""
    q, r, ex = _pair(queries, refs, exclude_self)
    Nq, Lz = q.shape
    Nr = r.shape[0]
    cand = torch.as_tensor(cand).to(q.device)
    if cand.dim() != 2 or cand.shape[0] != Nq or cand.dtype.is_floating_point:
        raise ValueError(f"cand must be an integer tensor [{Nq}, m]")
    m = _check_count(cand.shape[1], "m")
    cand = cand.to(torch.int32).contiguous()
    rows = _rows(rows, Nq, Nr)
    ws = torch.empty(workspace_bytes(rows, Nr, Lz), dtype=torch.uint8, device=q.device)
    out = torch.empty(Nq, m, dtype=torch.int32, device=q.device)
    for r0 in range(0, Nq, rows):
        n = min(rows, Nq - r0)
        L.check(L.lib.gmvae_knn_ranks(L.ptr(q[r0:]), n, L.ptr(r), Nr, Lz, r0 if ex else -1, L.ptr(cand[r0:]), m, L.ptr(out[r0:]),
                                      L.ptr(ws), L.current_stream()), "gmvae_knn_ranks")
    return out


def class_sums(queries, refs, labels, n_labels, rows=None):
    """S [Nq, n_labels] (fp64): S[i, c] = the sum of the distances (not squared) from query i to the references labelled c.  A
    label outside [0, n_labels) contributes nowhere; self is not excluded."""
    q, r, _ = _pair(queries, refs, False)
    Nq, Lz = q.shape
    Nr = r.shape[0]
    n_labels = _check_count(n_labels, "n_labels", MAX_C)
    labels = _labels(labels, Nr)
    rows = _rows(rows, Nq, Nr)
    ws = torch.empty(workspace_bytes(rows, Nr, Lz, 1, n_labels), dtype=torch.uint8, device=q.device)
    out = torch.empty(Nq, n_labels, dtype=torch.float64, device=q.device)
    for r0 in range(0, Nq, rows):
        n = min(rows, Nq - r0)
        L.check(L.lib.gmvae_knn_class_sums(L.ptr(q[r0:]), n, L.ptr(r), Nr, Lz, L.ptr(labels), n_labels, L.ptr(out[r0:]), L.ptr(ws),
                                           L.current_stream()), "gmvae_knn_class_sums")
    return out


def _counts(index, valid, size):
    """Occurrences of index (int64, where valid) in [0, size): integer scatter-adds, so the same bits every run."""
    out = torch.zeros(size, dtype=torch.int64, device=index.device)
    return out.scatter_add_(0, torch.where(valid, index, torch.zeros_like(index)), valid.to(torch.int64))


def _votes(ref_labels, idx, n_labels):
    lab = ref_labels.long()[idx.long()]                                       # [Nq, k]
    valid = (lab >= 0) & (lab < n_labels)
    row = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand_as(lab)
    return _counts((row * n_labels + lab).reshape(-1), valid.reshape(-1), idx.shape[0] * n_labels).view(idx.shape[0], n_labels)


def _predict(votes):
    """The largest vote, ties to the smallest label (scikit-learn's rule for uniform weights)."""
    n = votes.shape[1]
    return (votes * n + (n - 1 - torch.arange(n, device=votes.device))).argmax(dim=1)


def knn_classify(ref_codes, ref_labels, query_codes, k, n_labels, exclude_self=False, rows=None):
    """The k-NN classifier: a dict of `pred` [Nq] (int64) and `votes` [Nq, n_labels] (int64), votes[i, c] = the number of query i's
    k nearest references labelled c.  A reference label outside [0, n_labels) votes for nothing."""
    n_labels = _check_count(n_labels, "n_labels", MAX_C)
    r = _codes(ref_codes, "ref_codes")
    ref_labels = _labels(ref_labels, r.shape[0], "ref_labels")
    idx = knn(query_codes, r, k, exclude_self=exclude_self, rows=rows)["idx"]
    votes = _votes(ref_labels, idx, n_labels)
    return {"pred": _predict(votes), "votes": votes}


def knn_accuracy(ref_codes, ref_labels, query_codes, query_labels, k, n_labels, rows=None):
    """The share of held-out queries whose k-NN prediction is their label: a 0-d tensor."""
    pred = knn_classify(ref_codes, ref_labels, query_codes, k, n_labels, rows=rows)["pred"]
    query_labels = _labels(query_labels, pred.shape[0], "query_labels")
    return (pred == query_labels.long()).double().mean()


def knn_accuracy_loo(codes, labels, k, n_labels, rows=None):
    """Leave-one-out k-NN accuracy of a labelled code (every example classified by the others): a 0-d tensor."""
    return knn_loo(codes, labels, k, n_labels, rows)["accuracy"]


def knn_loo(codes, labels, k, n_labels, rows=None):
    codes = _codes(codes)
    labels = _labels(labels, codes.shape[0])
    o = knn_classify(codes, labels, codes, k, n_labels, exclude_self=True, rows=rows)
    o["accuracy"] = (o["pred"] == labels.long()).double().mean()
    return o


def silhouette(codes, labels, n_labels, rows=None):
    """scikit-learn's silhouette of a labelling on the codes: a dict of `samples` [N] (fp64) and `score` (their mean, 0-d).  With
    n_c the class counts: a_i = S[i, c_i] / (n_{c_i} - 1), b_i = min over the other non-empty classes of S[i, c] / n_c, s_i =
    (b_i - a_i) / max(a_i, b_i); s_i = 0 in a class of one and where max(a_i, b_i) = 0.  An example labelled outside [0, n_labels)
    belongs to no class: NaN, and left out of the mean.  Fewer than two non-empty classes: the score is NaN."""
    codes = _codes(codes)
    N = codes.shape[0]
    n_labels = _check_count(n_labels, "n_labels", MAX_C)
    labels = _labels(labels, N)
    S = class_sums(codes, codes, labels, n_labels, rows)
    lab = labels.long()
    valid = (lab >= 0) & (lab < n_labels)
    n = _counts(lab, valid, n_labels).double()                               # [C]
    own = torch.where(valid, lab, torch.zeros_like(lab))
    n_own = n[own]
    a = S.gather(1, own.unsqueeze(1)).squeeze(1) / (n_own - 1)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=S.device)
    other = torch.arange(n_labels, device=S.device).unsqueeze(0) != own.unsqueeze(1)
    b = torch.where(other & (n > 0).unsqueeze(0), S / n.unsqueeze(0), inf).min(dim=1).values
    m = torch.maximum(a, b)
    s = torch.where((n_own == 1) | (m == 0), torch.zeros_like(m), (b - a) / m)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=S.device)
    s = torch.where(valid, s, nan)
    score = torch.where(valid, s, torch.zeros_like(s)).sum() / valid.sum()
    return {"samples": s, "score": torch.where((n > 0).sum() >= 2, score, nan)}


def trustworthiness(codes, embedding, k=5, rows=None):
    """T(k) = 1 - 2 / (N k (2N - 3k - 1)) sum_i sum_t max(0, rank_X(i, knn_Y[i, t]) - k + 1): how far the embedding Y's k nearest
    neighbours are neighbours in the codes X (scikit-learn's manifold.trustworthiness on data without distance ties); k < N / 2.
    A 0-d fp64 tensor."""
    X, Y = _codes(codes), _codes(embedding, "embedding")
    N = X.shape[0]
    k = _check_count(k, "k")
    if Y.shape[0] != N:
        raise ValueError(f"codes and embedding differ in N: {N} and {Y.shape[0]}")
    if not k < N / 2:
        raise ValueError(f"k must be below N / 2: k = {k}, N = {N}")
    rk = ranks(X, X, knn(Y, k=k, rows=rows)["idx"], exclude_self=True, rows=rows).long()
    penalty = (rk - (k - 1)).clamp_min(0).sum().double()
    return 1.0 - penalty * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def continuity(codes, embedding, k=5, rows=None):
    """Trustworthiness with the two spaces exchanged: how far the codes' neighbours stay neighbours in the embedding."""
    return trustworthiness(embedding, codes, k, rows)


def contingency(a, b, n_a, n_b):
    """[n_a, n_b] (fp64) counts of the pairs (a_i, b_i); a pair with either label out of range is left out."""
    n_a, n_b = int(n_a), int(n_b)
    if n_a < 1 or n_b < 1:
        raise ValueError("n_a and n_b must be >= 1")
    a = torch.as_tensor(a).to(L.require_gpu())
    if a.dim() != 1:
        raise ValueError("a and b must be integer tensors [N]")
    a, b = _labels(a, a.shape[0], "a").long(), _labels(b, a.shape[0], "b").long()
    valid = (a >= 0) & (a < n_a) & (b >= 0) & (b < n_b)
    return _counts(a * n_b + b, valid, n_a * n_b).view(n_a, n_b).double()


def _entropy(c, n):
    return -torch.where(c > 0, c / n * (torch.log(c.clamp_min(1.0)) - torch.log(n)), torch.zeros_like(c)).sum()


def nmi(a, b, n_a, n_b):
    """Normalised mutual information of two labellings, arithmetic normalisation (scikit-learn's normalized_mutual_info_score):
    a 0-d fp64 tensor.  1 when each labelling is a single class, 0 when the mutual information is not positive."""
    t = contingency(a, b, n_a, n_b)
    n = t.sum()
    ra, rb = t.sum(dim=1), t.sum(dim=0)
    logt, logn = torch.log(t.clamp_min(1.0)), torch.log(n)
    outer = torch.log((ra.unsqueeze(1) * rb.unsqueeze(0)).clamp_min(1.0))
    mi = torch.where(t > 0, t / n * (logt - logn) + t / n * (2.0 * logn - outer), torch.zeros_like(t)).sum()
    h = 0.5 * (_entropy(ra, n) + _entropy(rb, n))
    one, zero = torch.ones_like(mi), torch.zeros_like(mi)
    single = ((ra > 0).sum() == 1) & ((rb > 0).sum() == 1)
    return torch.where(single, one, torch.where(mi > 0, mi / h, zero))


def ari(a, b, n_a, n_b):
    """Adjusted Rand index of two labellings (scikit-learn's adjusted_rand_score): a 0-d fp64 tensor."""
    t = contingency(a, b, n_a, n_b)
    n = t.sum()
    sq = (t * t).sum()
    tp, fp, fn = sq - n, (t.sum(dim=0) ** 2).sum() - sq, (t.sum(dim=1) ** 2).sum() - sq
    tn = n * n - fp - fn - sq
    den = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)
    perfect = (fn == 0) & (fp == 0)
    return torch.where(perfect, torch.ones_like(n), 2.0 * (tp * tn - fn * fp) / torch.where(perfect, torch.ones_like(den), den))


def scores(codes, labels=None, clusters=None, k=10, n_labels=10, n_clusters=None, rows=None):
    """The scores of one code: with `labels` knn_acc_loo, knn_pred [N], silhouette_labels and silhouette_labels_samples [N]; with
    `clusters` (an int tensor [N], n_clusters classes) silhouette_clusters and silhouette_clusters_samples; with both nmi and ari."""
    codes = _codes(codes)
    out = {}
    if labels is not None:
        loo = knn_loo(codes, labels, k, n_labels, rows)
        sil = silhouette(codes, labels, n_labels, rows)
        out.update(knn_acc_loo=loo["accuracy"], knn_pred=loo["pred"], silhouette_labels=sil["score"],
                   silhouette_labels_samples=sil["samples"])
    if clusters is not None:
        if n_clusters is None:
            raise ValueError("n_clusters is required with clusters")
        sil = silhouette(codes, clusters, n_clusters, rows)
        out.update(silhouette_clusters=sil["score"], silhouette_clusters_samples=sil["samples"])
        if labels is not None:
            out.update(nmi=nmi(labels, clusters, n_labels, n_clusters), ari=ari(labels, clusters, n_labels, n_clusters))
    return out


def model_scores(model, images, labels=None, clusters=None, k=10, n_labels=10, n_clusters=None, cluster_samples=16):
    """model.neighbour_scores: scores(model.transform(images), ...).  clusters None: the model's own clustering where it has one --
    the GMVAE's argmax q(y | x), the mixture-prior VAE's predict_clusters(images, cluster_samples) -- over its mixture_components
    classes; a plain VAE has none."""
    mix = int(getattr(model, "mix_components", 1) or 1)
    if clusters is None and mix > 1:
        if hasattr(model, "encoder_y"):
            clusters = model.encoder_y(images).distribution.logits.argmax(dim=1)
        else:
            clusters = model.predict_clusters(images, int(cluster_samples))
    if clusters is not None and n_clusters is None:
        n_clusters = mix if mix > 1 else None
    return scores(model.transform(images), labels, clusters, k=k, n_labels=n_labels, n_clusters=n_clusters)
