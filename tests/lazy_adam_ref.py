"""The lazy train step's reference in fp64 (kge_train_step_lazy; tests/test_lazy_adam_cpu.py holds it to
torch.optim.SparseAdam, tests/test_lazy_adam_gpu.py holds the library to it). A plain module: nothing here is a
fixture or changes how the suite is collected.

A row is touched when the batch names it: an entity by an in-range id among the negatives, the positive heads or
the positive tails, a relation by some pos[b, 1]. Touched rows get the dense Adam update (Keras or torch rule, the
global step number t in the bias correction); untouched rows keep their parameter and both moments."""
import torch

from oracle import kge_oracle as O

B1, B2 = 0.9, 0.999


def touched_masks(pos, neg, E, R):
    """(entity [E], relation [R]) bool masks of the rows a batch touches; out-of-range entity ids are dropped."""
    ids = torch.cat([neg.reshape(-1), pos[:, 0], pos[:, 2]])
    ids = ids[(ids >= 0) & (ids < E)]
    ent = torch.zeros(E, dtype=torch.bool)
    ent[ids] = True
    rel = torch.zeros(R, dtype=torch.bool)
    rid = pos[:, 1]
    rel[rid[(rid >= 0) & (rid < R)]] = True
    return ent, rel


def torch_adam_step(p, g, m, v, t, lr, beta1=B1, beta2=B2, epsilon=1e-8):
    """torch.optim.Adam's update, dense form: eps is added to sqrt(v_hat). Returns (p, m, v)."""
    m = m + (g - m) * (1 - beta1)
    v = v + (g * g - v) * (1 - beta2)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    p = p - (lr / bc1) * m / (torch.sqrt(v) / bc2 ** 0.5 + epsilon)
    return p, m, v


def adam_rows(p, g, m, v, t, lr, mask=None, keras=True, epsilon=None):
    """One Adam step of the [rows, w] table p on the rows of `mask` (None: every row, the dense optimizer);
    the other rows keep p, m and v. Returns (p, m, v)."""
    if epsilon is None:
        epsilon = 1e-7 if keras else 1e-8
    rule = O.keras_adam_step if keras else torch_adam_step
    p2, m2, v2 = rule(p, g, m, v, t, lr, B1, B2, epsilon)
    if mask is None:
        return p2, m2, v2
    k = mask[:, None]
    return torch.where(k, p2, p), torch.where(k, m2, m), torch.where(k, v2, v)


def train_grads(name, ent, rel, pos, neg, w, mode, gamma, rng, upstream=False):
    """(loss, d_ent, d_rel) in fp64 by autograd: O.tf_train_loss (TFKGEModel.train_step_fused; mode 0 / 1), or
    O.upstream_train_loss with its defaults but uni_weight where w is None (KGEModel.train_step_fused)."""
    e, r = ent.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    if upstream:
        uni = w is None
        wt = torch.ones(pos.shape[0], dtype=torch.float64) if uni else w.double()
        loss = O.upstream_train_loss(name, e, r, pos, neg, wt, "head-batch" if mode == 0 else "tail-batch", gamma,
                                     rng, adversarial=True, temperature=1.0, uni_weight=uni)
    else:
        loss = O.tf_train_loss(name, e, r, pos, neg, w.double(), torch.tensor([mode] * pos.shape[0]), gamma, rng)
    loss.backward()
    return loss.item(), e.grad, r.grad


class RefStep:
    """The fp64 state (tables and moments) of one model and one reference step per step(): lazy (Adam on the
    touched rows only) or dense."""

    def __init__(self, name, ent, rel, gamma, rng, lr, keras=True, lazy=True, upstream=False):
        self.name, self.gamma, self.rng, self.lr = name, gamma, rng, lr
        self.keras, self.lazy, self.upstream = keras, lazy, upstream
        self.ent, self.rel = ent.double().clone(), rel.double().clone()
        self.mv = [torch.zeros_like(self.ent), torch.zeros_like(self.ent), torch.zeros_like(self.rel),
                   torch.zeros_like(self.rel)]
        self.t = 0

    def step(self, pos, neg, w, mode):
        loss, ge, gr = train_grads(self.name, self.ent, self.rel, pos, neg, w, mode, self.gamma, self.rng,
                                   self.upstream)
        me, mr = touched_masks(pos, neg, self.ent.shape[0], self.rel.shape[0]) if self.lazy else (None, None)
        self.t += 1
        self.ent, self.mv[0], self.mv[1] = adam_rows(self.ent, ge, self.mv[0], self.mv[1], self.t, self.lr, me,
                                                     self.keras)
        self.rel, self.mv[2], self.mv[3] = adam_rows(self.rel, gr, self.mv[2], self.mv[3], self.t, self.lr, mr,
                                                     self.keras)
        return loss
