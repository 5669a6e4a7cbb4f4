"""The mean teacher of Stage-2 consistency training (train_stage2.py:58-63, 302-312, 328-332): `EMA`, a restatement of
`ema_pytorch.EMA` 0.2.3 at its defaults.  The package is installed on no machine of this project: what is
written here follows its published source as read, and has NOT been compared with it.  Every constant is a constructor keyword
with the package's name and default, so that someone who has the package can align the two.

    ema = EMA(model)            # a deep copy, requires_grad off, module modes as copied and never changed
    ema.bind(optimizer)         # optional: the teacher's arena parameters move into mirror arenas (one launch per arena)
    maps = ema(img, word_ids)   # the copy's forward
    ema.update()                # after optimizer.step()

update() reads `step`, increments it, and then: returns if step % update_every != 0; copies student -> teacher and returns if
step <= update_after_step; otherwise copies once more the first time it gets here, and then, for every floating-point parameter
and buffer by name, teacher.lerp_(student, 1 - decay), decay = get_current_decay() at the incremented step.  Integer buffers
(num_batches_tracked) are never touched.  The schedule and the copy / lerp / skip decision are host code (`_advance`); the launches
are ops.ema_update (csrc/seg.hip: tris_lerp_f32 / tris_lerp_table_f32), a copy being a lerp of weight 1.
"""
import copy

import torch
from torch import nn

from . import ops
from .optim import Arena

_STATIC_FLAGS = ("_tris_no_grad_path", "_tris_linear_w", "_tris_accumulates")   # a deep copy of a Parameter drops its attributes


class _MirrorArena:
    """the teacher's copies of one optimiser arena's parameters in one flat buffer with that arena's offsets -- what
    ops.h2_register_arena and ops.h2_weights_amax read of an arena (.p, .params, .offsets)"""

    def __init__(self, arena, params):
        self.params, self.offsets, self.numel = list(params), list(arena.offsets), arena.numel
        self.p = torch.zeros_like(arena.p)
        for p, o in zip(self.params, self.offsets):
            v = Arena._view(self.p, p, o)
            with torch.no_grad():
                v.copy_(p.data)
            p.data = v


class EMA(nn.Module):
    def __init__(self, model, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2 / 3, min_value=0.0):
        super().__init__()
        self.beta, self.update_after_step, self.update_every = beta, update_after_step, update_every
        self.inv_gamma, self.power, self.min_value = inv_gamma, power, min_value
        self.ema_model = copy.deepcopy(model)
        self.ema_model.requires_grad_(False)
        self.__dict__["online_model"] = model          # (not a submodule: the student's parameters are not this module's)
        src = dict(model.named_parameters())
        for k, p in self.ema_model.named_parameters():
            for flag in _STATIC_FLAGS:
                if hasattr(src[k], flag):
                    setattr(p, flag, getattr(src[k], flag))
        self.step, self.initted = 0, False
        self._arenas = []          # [(mirror arena, optimiser arena)] once bound
        self._table = None

    # ---------------------------------------------------------------------------------------------------------- host logic
    def covered_names(self):
        """names of the tensors update() writes: every floating-point parameter and buffer of the copy"""
        m = self.ema_model
        return [k for k, t in list(m.named_parameters()) + list(m.named_buffers()) if t.is_floating_point()]

    def get_current_decay(self):
        epoch = max(self.step - self.update_after_step - 1, 0)
        if epoch <= 0:
            return 0.0
        value = 1 - (1 + epoch / self.inv_gamma) ** -self.power
        return min(max(value, self.min_value), self.beta)

    def _advance(self):
        """one update() on the host: -> the lerp weights to launch, in order ([] = skipped, 1.0 = the copy, 1 - decay)"""
        step = self.step
        self.step += 1
        if step % self.update_every != 0:
            return []
        if step <= self.update_after_step:
            return [1.0]
        out = []
        if not self.initted:
            out.append(1.0)
            self.initted = True
        out.append(1.0 - self.get_current_decay())
        return out

    def update(self, *args):
        if args:
            raise TypeError(f"update() takes no argument ({len(args)} given): the student is the model this EMA was built from")
        for w in self._advance():
            self._launch(w)

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)

    # ---------------------------------------------------------------------------------------------------------- device side
    def bind(self, optimizer):
        """Move the teacher's copies of the optimiser's arena parameters into mirror arenas: an update is then one launch per arena
        plus one for the rest (BatchNorm buffers, parameters outside the arenas), and the teacher's weights get their h2 amax words
        as the student's do, from one launch per arena and step."""
        if self._arenas:
            raise RuntimeError("this EMA is already bound to an optimiser")
        name_of = {id(p): k for k, p in self.online_model.named_parameters()}
        mine = dict(self.ema_model.named_parameters())
        pairs = []
        for a in optimizer.arenas:
            missing = [p for p in a.params if id(p) not in name_of]
            if missing:
                raise ValueError(f"{len(missing)} parameters of the optimiser do not belong to the model this EMA was built from")
            pairs.append((_MirrorArena(a, [mine[name_of[id(p)]] for p in a.params]), a))
        words = sum(len(m.params) + len(a.params) for m, a in pairs)
        if words > ops.H2_SLOTS // 2:
            raise RuntimeError(f"the h2 amax pool holds {ops.H2_SLOTS // 2} weight words, the student's and the teacher's arenas need "
                               f"{words}: one of them would silently lose its amax words")
        for m, _ in pairs:
            ops.h2_register_arena(m)
        self._arenas, self._table = pairs, None

    def _pairs_outside_arenas(self):
        inside = {id(p) for m, _ in self._arenas for p in m.params}
        s, t = self.online_model, self.ema_model
        src = dict(list(s.named_parameters()) + list(s.named_buffers()))
        dst = dict(list(t.named_parameters()) + list(t.named_buffers()))
        return [(dst[k], src[k]) for k in self.covered_names() if id(dst[k]) not in inside]

    def _launch(self, w):
        pairs = self._pairs_outside_arenas()
        held = self._table.pairs if self._table is not None else ()
        if len(held) != len(pairs) or any(d.data_ptr() != d0.data_ptr() or s.data_ptr() != s0.data_ptr()
                                          for (d, s), (d0, s0) in zip(pairs, held)):
            # (first update, or a tensor has moved since: .cuda(), an optimiser built after the last update)
            self._table = ops.LerpTable([(d.detach(), s.detach()) for d, s in pairs])
        for m, a in self._arenas:
            if a.params[0].data_ptr() != a.p.data_ptr() + 4 * a.offsets[0]:
                raise RuntimeError("the optimiser this EMA is bound to no longer owns the student's parameters")
        ops.ema_update([(m.p, a.p) for m, a in self._arenas], w)
        ops.ema_update(self._table, w)
        # the kernels write in place without telling torch: constant amax words (ops._h2_const_slot) are keyed on the version
        torch.autograd.graph.increment_version([d for d, _ in self._table.pairs])
