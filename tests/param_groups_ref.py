"""What a grouped AdamW step must give, composed from the update WITHOUT groups.  TEST INFRASTRUCTURE ONLY.

AdamW is element-wise: element i of an arena stepped with parameter groups gets what the whole arena stepped with the (lr, weight_decay)
of i's group gives it.  So the reference of nv_adamw_step_grouped is the existing kernel - one ops.adamw_step over a clone of the arena
per group, element i taken from the run of its own group (`compose_device`) - and the two must agree bit for bit.  `compose_host` is the
same composition on the CPU over oracle.train_step.AdamW; tests/test_param_groups_cpu.py proves it against torch.optim.AdamW with real
parameter groups.
"""
import torch

from oracle import train_step


def element_groups(ends, index, total=None) -> torch.Tensor:
    """int64 [total]: the group of every element, from the segment table (ends ascending, group index per segment)"""
    total = ends[-1] if total is None else total
    out = torch.empty(total, dtype=torch.int64)
    at = 0
    for end, g in zip(ends, index):
        out[at:end] = g
        at = end
    assert at == total
    return out


def compose_device(ops, p, grad, m, v, p16, step, elem_group, lrs, wds, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_blocks=0,
                   scale_state=None, clip_state=None):
    """(p, m, v, p16) after one step, from one ops.adamw_step run per group over clones of (p, m, v, p16); the inputs are not written.
    scale_state: the loss-scale block as it is BEFORE nv_loss_scale_update - each group's run gets its own clone, updated with its lr."""
    eg = elem_group.to(p.device)
    out = [p.clone(), m.clone(), v.clone(), None if p16 is None else p16.clone()]
    for g, (lr, wd) in enumerate(zip(lrs, wds)):
        run = [p.clone(), m.clone(), v.clone(), None if p16 is None else p16.clone()]
        st = None
        if scale_state is not None:
            st = scale_state.clone()
            ops.loss_scale_update(st, lr, betas)
        ops.adamw_step(run[0], grad, run[1], run[2], run[3], step, lr, betas, eps, wd, grad_scale, max_blocks, scale_state=st, clip_state=clip_state)
        mine = eg == g
        for o, r in zip(out, run):
            if o is not None:
                o[mine] = r[mine]
    return out


def compose_host(p, grad, m, v, t, elem_group, lrs, wds, betas=(0.9, 0.999), eps=1e-8):
    """(p, m, v) after AdamW step t + 1 on the CPU: one oracle AdamW per group over clones, element i from its own group's run"""
    out = [p.clone(), m.clone(), v.clone()]
    for g, (lr, wd) in enumerate(zip(lrs, wds)):
        opt = train_step.AdamW({"w": p.clone()}, lr=lr, betas=betas, eps=eps, weight_decay=wd)
        opt.m["w"], opt.v["w"], opt.t = m.clone(), v.clone(), t
        opt.step({"w": grad})
        mine = elem_group == g
        for o, r in zip(out, (opt.params["w"], opt.m["w"], opt.v["w"])):
            o[mine] = r[mine]
    return out
