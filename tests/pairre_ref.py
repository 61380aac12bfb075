"""The fp64 reference of the PairRE score function (Chao et al. 2021), restated from its definition:

    r_h, r_t = relation[:, :D], relation[:, D:2D]
    h^ = h / max(||h||_2, 1e-12)      t^ = t / max(||t||_2, 1e-12)
    score = gamma - sum_i | h^_i r_h,i - t^_i r_t,i |

the same formula in all three modes. An out-of-range entity or relation id reads a zero row (the library's contract).
Gradients are autograd's of this restatement; the losses are supervisor.py:17-23 / upstream's train_step over
oracle.kge_oracle's reductions, which take scores. A plain module: nothing here is a fixture."""
import torch
import torch.nn.functional as F

from oracle import kge_oracle as O

EPS = 1e-12


def normalize(x):
    return x / x.norm(p=2, dim=-1, keepdim=True).clamp_min(EPS)


def rows(table, ids):
    """table[ids] with a zero row for every id outside [0, rows)."""
    ok = (ids >= 0) & (ids < table.shape[0])
    return table[ids.clamp(0, table.shape[0] - 1)] * ok.unsqueeze(-1).to(table.dtype)


def score_rows(head, relation, tail, gamma):
    D = head.shape[-1]
    assert relation.shape[-1] >= 2 * D
    r_h, r_t = relation[..., :D], relation[..., D:2 * D]
    return gamma - (normalize(head) * r_h - normalize(tail) * r_t).abs().sum(-1)


def score(ent, rel, pos, neg, mode, gamma):
    """Raw scores [B, N] of head-batch (mode 0) / tail-batch (1) candidates neg, or [B, 1] of the positives (3)."""
    h, r, t = rows(ent, pos[:, 0]).unsqueeze(1), rows(rel, pos[:, 1]).unsqueeze(1), rows(ent, pos[:, 2]).unsqueeze(1)
    if mode == 0:
        h = rows(ent, neg)
    elif mode == 1:
        t = rows(ent, neg)
    else:
        assert mode == 3
    return score_rows(h, r, t, gamma)


def score_all(ent, rel, pos, mode, gamma, chunk=8):
    """[B, E] scores of every entity as the candidate, a few query rows at a time."""
    E = ent.shape[0]
    out = []
    for s in range(0, pos.shape[0], chunk):
        p = pos[s:s + chunk]
        out.append(score(ent, rel, p, torch.arange(E).unsqueeze(0).expand(len(p), E), mode, gamma))
    return torch.cat(out)


def reduced(ent, rel, pos, neg, mode, gamma, red="tf", T=1.0):
    """(reduced negative branch [B], logsigmoid of the positive score [B], negative scores [B, N], positive [B])."""
    s = score(ent, rel, pos, neg, mode, gamma)
    ps = score(ent, rel, pos, neg, 3, gamma)[:, 0]
    if red == "tf":
        n = O.adv_reduce(s, T)[:, 0]
    elif red == "mean":
        n = O.mean_reduce(s)[:, 0]
    else:
        assert red == "detached"
        n = (torch.softmax(s * T, dim=1).detach() * F.logsigmoid(-s)).sum(dim=1)
    return n, F.logsigmoid(ps), s, ps


def train_loss(ent, rel, pos, neg, w, mode, gamma, red="tf", T=1.0, lam=0.0):
    """supervisor.py:17-23 (red "tf") or upstream's loss (red "detached" / "mean"), w None: plain means; lam: the
    L3 regulariser's weight. Returns (loss, positive_sample_loss, negative_sample_loss)."""
    n, p, _, _ = reduced(ent, rel, pos, neg, mode, gamma, red, T)
    w = torch.ones_like(n) if w is None else w.reshape(-1).to(n.dtype)
    pl, nl = -(w * p).sum() / w.sum(), -(w * n).sum() / w.sum()
    loss = (pl + nl) / 2
    if lam:
        loss = loss + lam * ((ent.abs() ** 3).sum() + (rel.abs() ** 3).sum())
    return loss, pl, nl


def train_grads(ent, rel, pos, neg, w, mode, gamma, red="tf", T=1.0, lam=0.0):
    """(loss, d_ent, d_rel) of train_loss at the fp64 tables ent, rel."""
    e, r = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    loss, _, _ = train_loss(e, r, pos, neg, w, mode, gamma, red, T, lam)
    loss.backward()
    return float(loss.detach()), e.grad, r.grad
