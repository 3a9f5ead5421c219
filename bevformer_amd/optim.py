"""``AdamW2`` (also ``FusedAdamW``): gradient-norm clipping + AdamW as two HIP launches per step (csrc/optim.h).

What every reference config runs after the backward — ``clip_grad_norm_(max_norm=35, norm_type=2)``, then AdamW with
``lr=2e-4``, ``weight_decay=0.01`` (projects/configs/bevformer/bevformer_base.py:228-244; the plugin registers its own copy of
torch's AdamW as ``AdamW2``: projects/mmdet3d_plugin/models/opt/adamw.py) — with every scalar of the step on the device: the
norm, the clip coefficient, each parameter's step count, the groups' hyperparameters.  ``step()`` reads nothing back, so it can
be captured in a HIP graph together with the forward, the loss and the backward.

    opt = AdamW2(model.parameters(), lr=2e-4, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2))
    loss.backward(); opt.step(); opt.zero_grad()          # opt.grad_norm: the 0-d device tensor clip_grad_norm_ returns

Contract of a captured ``step()``: the job table (addresses of parameters, gradients and state) and the hyperparameters are
what they were at capture; a schedule that rewrites ``group['lr']`` calls ``opt.sync_hyperparameters()`` between replays (an
upload on the current stream) — nothing is uploaded by ``step()`` while a capture is under way.  ``state_dict()`` has
``torch.optim.AdamW``'s layout (``step`` as 0-d float32 CPU tensors: one device-to-host copy), ``load_state_dict()`` takes
torch's — ``step`` as an int (torch 1.9, the reference's checkpoints), a float or a tensor.  Anything the kernels do not
cover raises with the reason of ``ops.fused_reject``: there is no fallback to torch's update."""
import torch

from . import ops
from .registry import OPTIMIZERS


@OPTIMIZERS.register_module(name="AdamW2", force=True)
class AdamW2(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, grad_clip=None,
                 skip_nonfinite=False):
        for name, v in (("lr", lr), ("eps", eps), ("weight_decay", weight_decay), ("beta1", betas[0]), ("beta2", betas[1])):
            if isinstance(v, torch.Tensor):
                raise ValueError(f"AdamW2: {name} must be a Python number (the device copy is made by the optimizer)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # (the keys of torch.optim.AdamW's groups, so that a state_dict of this class loads there and runs as AdamW)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        self.grad_clip = None if grad_clip is None else dict(grad_clip)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._steps = None            # every parameter's step count: ONE flat float32 device tensor
        self._slot = {}               # id(parameter) -> its index in _steps
        self._scalars = None          # the 8 words of csrc/optim.h: total_norm, clip_coef, skip, skipped, ticket
        self._groups_dev = None       # (ngroups, 5) float64: lr, beta1, beta2, eps, weight_decay
        self._groups_host = None      # ... and the host values it was uploaded from
        self._table = None            # dict(key, table, staging, workspace, njobs, blocks, params): never rewritten
        self._frozen = []             # tables and staging buffers a captured graph reads: kept alive, never rewritten
        self._spare = None            # a pinned staging buffer made OUTSIDE a capture for the table a capture may build
        self._constructed = False
        super().__init__(params, defaults)
        self._constructed = True
        self._check()

    # ---- what the kernels cover
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _check(self, check_grads=False):
        reason = ops.fused_reject(self._params(), amsgrad=any(g["amsgrad"] for g in self.param_groups),
                                  maximize=any(g.get("maximize", False) for g in self.param_groups),
                                  grad_clip=self.grad_clip, check_grads=check_grads)
        if reason is None and any(not g.get("decoupled_weight_decay", True) for g in self.param_groups):
            reason = "decoupled_weight_decay=False (Adam's L2 penalty) is not implemented by the device kernels"
        if reason is not None:
            raise RuntimeError(f"AdamW2: {reason}")

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:     # (a torch 1.9 checkpoint's groups carry lr, betas, eps, weight_decay, amsgrad only)
            for k, v in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                         ("differentiable", False), ("fused", None), ("decoupled_weight_decay", True)):
                g.setdefault(k, v)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if self._constructed:
            self._check()
            self._table = None

    # ---- device state
    @property
    def device(self):
        return self._params()[0].device

    def _ensure_buffers(self):
        params = self._params()
        if self._scalars is None:
            self._scalars = torch.zeros(8, dtype=torch.float32, device=self.device)
        if self._steps is None or self._steps.numel() != len(params) or any(id(p) not in self._slot for p in params):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("AdamW2: the optimizer's state cannot be created inside a stream capture: run one eager "
                                   "step() (or load_state_dict) first")
            steps = torch.zeros(len(params), dtype=torch.float32, device=self.device)
            old, old_slot = self._steps, self._slot
            self._slot = {id(p): i for i, p in enumerate(params)}
            if old is not None:
                keep = [(self._slot[k], i) for k, i in old_slot.items() if k in self._slot]
                if keep:
                    steps[[a for a, _ in keep]] = old[[b for _, b in keep]]
            self._steps = steps
            for p in params:            # ('step' of a parameter's state: a 0-d view of the flat tensor)
                if p in self.state and "step" in self.state[p]:
                    self.state[p]["step"] = self._steps[self._slot[id(p)]]
            self._table = None
        if self._spare is None and not torch.cuda.is_current_stream_capturing():
            self._spare = torch.empty((len(params), ops.OPTIM_JOB_WORDS), dtype=torch.int64).pin_memory()

    @property
    def grad_norm(self):
        """The total 2-norm of the gradients of the last ``step()``, before clipping: a 0-d float32 DEVICE tensor."""
        self._ensure_buffers()
        return self._scalars[0]

    @property
    def clip_coef(self):
        """The factor the last ``step()`` scaled every gradient by: a 0-d float32 DEVICE tensor."""
        self._ensure_buffers()
        return self._scalars[1]

    @property
    def skipped_steps(self):
        """Steps skipped for a non-finite gradient norm (``skip_nonfinite=True``): a 0-d int32 DEVICE tensor."""
        self._ensure_buffers()
        return self._scalars.view(torch.int32)[3]

    def _hyper(self):
        return tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
                     for g in self.param_groups)

    def sync_hyperparameters(self, force=False):
        """Upload the groups' ``lr``, ``betas``, ``eps``, ``weight_decay`` on the current stream when the host values changed
        (``force``: anyway).  ``step()`` does this itself except during a stream capture; between the replays of a captured
        step it is the caller's (a replayed graph reads the device copy as it is then)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AdamW2.sync_hyperparameters: called during a stream capture (the upload would be frozen "
                               "into the graph); call it between replays")
        host = self._hyper()
        if not force and self._groups_dev is not None and host == self._groups_host:
            return False
        if self._groups_dev is None or self._groups_dev.shape[0] != len(host):
            self._groups_dev = torch.empty((len(host), ops.OPTIM_GROUP_WORDS), dtype=torch.float64, device=self.device)
            self._table = None
        staging = torch.tensor(host, dtype=torch.float64).reshape(len(host), ops.OPTIM_GROUP_WORDS).pin_memory()
        self._groups_dev.copy_(staging, non_blocking=True)
        self._groups_host = host
        return True

    # ---- the job table
    def _state_of(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            # (lazily, as torch does: a parameter that never had a gradient has no state)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] = self._steps[self._slot[id(p)]]
        return st

    def _build_table(self, key, live):
        entries = []
        step_base, dev = self._steps.data_ptr(), self.device
        for gi, p in live:
            st = self._state_of(p)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if m.dtype != torch.float32 or v.dtype != torch.float32 or not m.is_contiguous() or not v.is_contiguous() \
                    or m.device != dev or v.device != dev or m.numel() != p.numel() or v.numel() != p.numel():
                raise RuntimeError("AdamW2: exp_avg / exp_avg_sq must be contiguous float32 tensors of the parameter's size "
                                   "on its device")
            entries.append((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), step_base + 4 * self._slot[id(p)],
                            p.numel(), gi))
        rows, blocks = ops.optim_job_rows(entries)
        # a pinned staging buffer and a device table of its own per rebuild: neither is ever rewritten, so a graph that
        # captured the copy (or launches that read the table) replays what it captured.  The staging buffer is the spare
        # made outside any capture (pinned memory is not allocated while a capture is under way), and the next spare is made
        # at once
        if self._spare is None or self._spare.shape[0] < len(rows):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("AdamW2: a second job table inside one stream capture (the gradients' addresses changed "
                                   "twice): capture one step() per graph")
            self._spare = torch.empty((len(self._slot), ops.OPTIM_JOB_WORDS), dtype=torch.int64).pin_memory()
        staging, self._spare = self._spare[:len(rows)], None
        staging.copy_(torch.tensor(rows, dtype=torch.int64).reshape(len(rows), ops.OPTIM_JOB_WORDS))
        if not torch.cuda.is_current_stream_capturing():
            self._spare = torch.empty((len(self._slot), ops.OPTIM_JOB_WORDS), dtype=torch.int64).pin_memory()
        table = torch.empty((len(rows), ops.OPTIM_JOB_WORDS), dtype=torch.int64, device=dev)
        table.copy_(staging, non_blocking=True)
        workspace = torch.empty(ops.optim_workspace_elems(blocks), dtype=torch.float64, device=dev)
        return dict(key=key, table=table, staging=staging, workspace=workspace, njobs=len(rows), blocks=blocks,
                    params=[p for _, p in live])

    @torch.no_grad()
    def step(self, closure=None):
        """One optimizer step on the current stream: the norm launch, the update launch, no host read.  Returns the
        closure's loss (or ``None``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ensure_buffers()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.sync_hyperparameters()
        elif self._groups_dev is None:
            raise RuntimeError("AdamW2: the first step() cannot be captured (nothing has been uploaded yet): run one eager "
                               "step() or sync_hyperparameters() before the capture")
        live = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"] if p.grad is not None]
        if not live:
            if not capturing:
                self._scalars[:2].zero_()
            return loss
        key = tuple((p.data_ptr(), p.grad.data_ptr(), gi) for gi, p in live)
        t = self._table
        if t is None or t["key"] != key:
            self._check(check_grads=True)
            if capturing and t is not None:
                self._frozen.append(t)          # (nothing pinned is released while a capture is under way)
            t = self._table = self._build_table(key, live)
        if capturing and not any(f is t for f in self._frozen):
            self._frozen.append(t)
        clip = self.grad_clip
        ops.optim_grad_norm(t["table"], t["njobs"], t["blocks"], t["workspace"], self._scalars,
                            max_norm=None if clip is None else clip["max_norm"], skip_nonfinite=self.skip_nonfinite)
        ops.optim_adamw(t["table"], t["njobs"], t["blocks"], self._groups_dev, self._groups_dev.shape[0], self._scalars)
        # the write the two launches made, told to the version counters: packed / panel / transposed weight images and
        # ops.graph_weights_stale() key on them (a skipped step bumps them too: an image rebuilt needlessly is still right)
        torch.autograd.graph.increment_version(t["params"])
        return loss

    def mark_replayed(self):
        """Tell the version counters of the parameters that a REPLAY of a captured ``step()`` wrote to them (host only, no
        launch): a replay runs no host code, so weight images cached per version for forwards OUTSIDE the graph — an
        evaluation between replays — would otherwise be taken for current.  The captured training step itself rebuilds its
        images inside the graph and does not need this."""
        params = [p for t in self._frozen for p in t["params"]]
        if params:
            torch.autograd.graph.increment_version(params)

    # ---- checkpoints in torch.optim.AdamW's layout
    def state_dict(self):
        sd = super().state_dict()
        if self._steps is not None and sd["state"]:
            steps = self._steps.detach().cpu()          # ONE device-to-host copy
            index = {}
            n = 0
            for g in self.param_groups:
                for p in g["params"]:
                    index[n] = self._slot.get(id(p))
                    n += 1
            for k, st in sd["state"].items():
                if "step" in st and index.get(k) is not None:
                    st = sd["state"][k] = dict(st)
                    st["step"] = steps[index[k]].clone()
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check()
        self._steps, self._slot, self._table = None, {}, None
        params = self._params()
        host = []
        for p in params:
            s = self.state[p].get("step", 0.0) if p in self.state else 0.0
            host.append(float(s.item()) if isinstance(s, torch.Tensor) else float(s))
        self._slot = {id(p): i for i, p in enumerate(params)}
        self._steps = torch.tensor(host, dtype=torch.float32).to(self.device)
        for p in params:
            if p in self.state and self.state[p]:
                st = self.state[p]
                st["step"] = self._steps[self._slot[id(p)]]
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self._groups_host = None


FusedAdamW = AdamW2
