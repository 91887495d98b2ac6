"""References shared by tests/test_head_train_cpu.py and tests/test_gpu_head_train.py: a numpy
restatement of Philox4x32-10 and of the dropout convention of include/pn2hip.h (pn2_dropout),
and TF's weighted sparse softmax cross-entropy (SUM_BY_NONZERO_WEIGHTS) in torch on the CPU."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter (n, 4), key (n, 2) or (2,) uint32 -> (n, 4) uint32 (Random123's philox4x32-10)."""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
    key = np.broadcast_to(np.asarray(key, np.uint64), c[0].shape + (2,))
    k0, k1 = key[..., 0] & MASK, key[..., 1] & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1,
             p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def dropout_keep(n, keep_prob, seed):
    """The keep mask of elements 0..n-1: key = (seed & 0xffffffff, seed >> 32), counter =
    (q & 0xffffffff, q >> 32, 0, 0) with q = e / 4, element e takes word e % 4, kept iff
    word < floor(keep_prob * 2^32) (keep_prob as the float32 the C ABI receives)."""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    counter = np.stack([q & MASK, q >> np.uint64(32), np.zeros_like(q), np.zeros_like(q)], axis=-1)
    key = np.array([seed & 0xffffffff, seed >> 32], np.uint64)
    words = philox4x32_10(counter, key).reshape(-1)[:n]
    thr = int(np.floor(float(np.float32(keep_prob)) * 2.0 ** 32))
    return words.astype(np.uint64) < np.uint64(thr)


def dropout_ref(x, keep_prob, seed):
    """x (float32 numpy, any shape) -> keep ? x / keep_prob : 0, the division in float32."""
    x = np.asarray(x, np.float32)
    keep = dropout_keep(x.size, keep_prob, seed).reshape(x.shape)
    return np.where(keep, x / np.float32(keep_prob), np.float32(0)).astype(np.float32)


def xent_ref(torch, logits, labels, weights, dt):
    """TF's reduction in dtype dt on the CPU: sum w (lse - z[label]) / count(w != 0), 0 without a
    present row. logits (rows, C), labels (rows) integer, weights (rows) or None. Returns (loss,
    lse, leaf logits): loss.backward() leaves the gradient in the leaf."""
    z = logits.detach().to(dt).clone().requires_grad_(True)
    lse = torch.logsumexp(z, dim=-1)
    ce = lse - z.gather(-1, labels.long().unsqueeze(-1)).squeeze(-1)
    w = torch.ones_like(ce) if weights is None else weights.to(dt)
    present = int((w != 0).sum())
    loss = (w * ce).sum() / present if present else (w * ce).sum() * 0
    return loss, lse, z
