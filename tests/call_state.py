"""TEST INFRASTRUCTURE: does a cached SamplerPlan carry anything from one call to the next?  Nothing in magicdrive_amd imports this.

A plan is built once and serves thousands of calls; between two calls stands only the hand-written list of copy_ / zero_ / fill_ in
SamplerPlan.load_inputs and ConditioningBuffers.load.  Two instruments, both bitwise (torch.equal, no tolerance anywhere):

  CPU   poison(plan) fills exactly the bytes the plan's programs write — the out_views and slack_views of tests/op_parity.py over prologue,
        step, jump and health ops, plus every scratch field whole — with NaN (floating-point storages) or 0x5A5A... (integer storages),
        and nothing else: weights, the tables written at build time and the pad channels of x_in stay.  load_inputs(B) and a run on the
        interpreter (tests/plan_interp.py) must then give what a freshly built plan gives for B.  A difference is a carry-over: bytes some
        op writes, load_inputs does not reset, and some op reads before this call has written them.  A wild integer is a Python exception
        on the interpreter, which fails the test too.  The integer poison exists HERE only: never in front of a kernel.  What no op
        writes is made stale the legal way: the test loads the inputs of call A in front of the poison.
  GPU   a real call A built to leave the worst state a call can leave (NaN latents in every scene, boxes at the capacity, every view given
        under fractional keep masks, its own seeds, eta, text and cameras), then call B on the same plan, against B on a fresh plan.
        NaN never becomes an address, and integer state ends where a finished call leaves it.

PLANS is the list both share; inputs(...) makes call A or B of a plan; state(...) is what is compared."""
import dataclasses

import torch

import op_parity as P
import plan_interp
from helpers import cfg_inputs, given_view_inputs, scene
from magicdrive_amd import denoiser as DN, ops as O, schedulers
from oracle import denoiser as D

HW = (28, 50)
INT_POISON = 0x5A5A5A5A5A5A5A5A              # outside every legal range of a counter, an index or a key count, at every width
RESAMPLE = (1, 2)                             # (jump length, samples): at 2 steps the shortest list with one jump and one revisited step

# name -> SamplerPlan switches (b = 1, no CFG, DDIM, box length 5 and 2 steps unless stated).  L_load: the box padding of call B on a
# dynamic plan whose capacity is L_box.
PLANS = {
    "ddim_cfg_fork": dict(do_cfg=True, fork=True),
    "unipc_given1": dict(sched="unipc", given=1),
    "given2": dict(given=2),
    "dynamic_boxes_cap8": dict(dynamic_boxes=True, L_box=8, L_load=3),
    "scene_boxes_b2": dict(b=2, dynamic_boxes="scene"),
    "health_trace": dict(health="trace"),
    "health_final": dict(health="final"),
    "regions": dict(given=1, keep_regions=True),
    "regions_resample": dict(given=1, keep_regions=True, resample=RESAMPLE[0]),
    "eta": dict(stochastic=True),
    "eta_regions_resample_trace": dict(given=1, keep_regions=True, resample=RESAMPLE[0], stochastic=True, health="trace"),
}
_NOT_PLAN_ARGS = ("b", "do_cfg", "sched", "given", "L_box", "L_load", "steps")


def interp(op):
    """The interpreter, one op.  It knows nothing of key counts: an attention that carries them is interpreted batch by batch over its first
    n keys (as tests/test_box_bucket.py does for tk_dev).  A count outside [1, Tk] — a poisoned one — is an error here."""
    if isinstance(op, O.Attn) and (op.tk_dev is not None or op.tk_rows is not None):
        B = op.Q.shape[0]
        counts = [int(op.tk_dev.item())] * B if op.tk_dev is not None else op.tk_rows.tolist()
        for b, n in enumerate(counts):
            assert 1 <= n <= op.Tk, f"{op.name}: key count {n} outside [1, {op.Tk}]"
            plan_interp.run([dataclasses.replace(op, Q=op.Q[b:b + 1], K=op.K[b:b + 1, :n], Vt=op.Vt[b:b + 1], O=op.O[b:b + 1], Tk=n, tk_dev=None, tk_rows=None)],
                            lower_check=False)
        return
    plan_interp.run([op], lower_check=False)


# ---- plans and calls ----------------------------------------------------------------------------------------------------------------------
def settings(which):
    """The switches of a plan: a name of PLANS, or a dict of the same form."""
    s = dict(b=1, do_cfg=False, sched="ddim", given=0, L_box=5, steps=2)
    s.update(PLANS[which] if isinstance(which, str) else which)
    s.setdefault("L_load", s["L_box"])
    return s


def build_plan(nets, which, dev, steps=None):
    """nets: (cfg, controlnet state dict, packed UNet, packed ControlNet) on `dev`."""
    cfg, _, un, cn = nets
    s = settings(which)
    kw = {k: v for k, v in s.items() if k not in _NOT_PLAN_ARGS}
    return DN.SamplerPlan(cfg, un, cn, dev, s["b"], s["do_cfg"], s["L_box"], HW, num_steps=steps or s["steps"], guidance_scale=2.0,
                          scheduler_kind=s["sched"], given_view_mode=s["given"], **kw)


def actions(which, steps=None):
    s = settings(which)
    n = steps or s["steps"]
    return schedulers.resample_actions(n, *RESAMPLE) if s.get("resample") else ["step"] * n


def _masks(given, seed):
    """fp32 (b, 6, 28, 50): on every given view a block of exact ones, a block of exact zeros and fractions elsewhere; zero on the others."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(*given.shape, *HW, generator=g)
    m[..., :9, :20] = 1.0
    m[..., 12:20, 25:] = 0.0
    return m * given[..., None, None]


def inputs(nets, which, variant, steps=None):
    """The arguments of load_inputs for call "A" (the dirty predecessor) or "B" (the call under test) of plan `which`."""
    cfg, csd, _, _ = nets
    s = settings(which)
    b, dirty = s["b"], variant == "A"
    n = steps or s["steps"]
    sc = scene(cfg, b, s["L_box"] if dirty else s["L_load"], HW, seed=4321 if dirty else 1234)
    sch = schedulers.DDIMScheduler() if s["sched"] == "ddim" else schedulers.UniPCMultistepScheduler()
    ts = sch.set_timesteps(n)
    if s["do_cfg"]:
        cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    else:
        cam, text, bev, boxes = sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"]
    lat = torch.stack([sc["latents"]] * 6, 1)
    if dirty:
        lat = torch.full_like(lat, float("nan"))
    kw = {}
    if s["given"]:
        g = torch.Generator().manual_seed(99 if dirty else 98)
        if dirty:                             # every view given
            gm = torch.ones(b, 6, dtype=torch.bool)
            gl = torch.randn(b, 6, 4, *HW, generator=g)
        else:                                 # one given view per scene
            cl = (given_view_inputs(HW) * b)[1:1 + b]
            gm = torch.tensor([[v is not None for v in r] for r in cl])
            gl = torch.stack([torch.stack([torch.zeros(4, *HW) if v is None else v for v in r]) for r in cl])
        kw.update(given_mask=gm, given_latents=gl)
        if s.get("keep_regions"):
            kw["keep_mask"] = _masks(gm, 7 if dirty else 5)
    if s.get("resample") or s.get("stochastic"):
        kw["seeds"] = torch.arange(b, dtype=torch.int64) * 7919 + (-(1 << 40) + 3 if dirty else (1 << 33) + 11)
    if s.get("stochastic"):
        kw["var"] = sch.variance_table(1.0 if dirty else 0.5)
    return (lat, cam, text, bev, boxes, ts, sch.coefficient_table()), kw


def run_interpreted(plan, acts, execute=interp):
    """prologue, the steps and jumps of `acts`, the health pass — on the CPU interpreter.  Returns the trail: state(plan) behind every
    action and behind the health pass (a call may end early: what it leaves then is visible too, e.g. the zero rows of a health trace)."""
    trail = []
    with torch.no_grad():
        for op in plan.prologue_ops:
            execute(op)
        for a in acts:
            for op in (plan.step_ops if a == "step" else plan.jump_ops):
                execute(op)
            trail.append(state(plan))
        for op in plan.health_ops:
            execute(op)
        trail.append(state(plan))
    return trail


def run_on_device(plan, acts):
    """The same on the GPU through the plan's own launchers: the step program is the captured graph (launch, not run); a forked plan replays
    its three parts on two streams."""
    if plan.prologue is None:
        plan.compile()
    main = torch.cuda.current_stream(plan.device)
    side = torch.cuda.Stream(plan.device) if plan.fork_at is not None else None
    st = main.cuda_stream
    trail = []
    plan.prologue.run(st)
    for a in acts:
        if a == "step":
            plan.launch_step(main, side, use_graph=True)
        else:
            plan.launch_jump(st, use_graph=True)
        trail.append(state(plan))
    plan.run_health(st)
    trail.append(state(plan))
    torch.cuda.synchronize(plan.device)
    return trail


def state(plan):
    """{name: clone} of everything a call leaves that the next caller can see: the latents, the model input, the health table, UniPC's
    history, the counters."""
    out = {"latents": plan.latents(), "x_in": plan.x_in.clone(), "step_ctr": plan.step_ctr.clone()}
    if plan.health_table() is not None:
        out["health"] = plan.health_table().clone()
    for name in ("x_last", "m1", "m2", "visit_ctr", "draw_ctr"):
        if hasattr(plan, name):
            out[name] = getattr(plan, name).clone()
    return out


def differences(got, want):
    """(position in the trail, name) of every quantity that is not bit-identical (torch.equal: a NaN anywhere is a difference)."""
    assert len(got) == len(want) and all(g.keys() == w.keys() for g, w in zip(got, want))
    return [(i, k) for i, (g, w) in enumerate(zip(got, want)) for k in sorted(g) if not torch.equal(g[k], w[k])]


# ---- the CPU poison -----------------------------------------------------------------------------------------------------------------------
def written_bytes(plan):
    """{storage: [a tensor on it, bool per byte]}: every byte some op of the plan's programs writes — op_parity.out_views (a GroupStats: the
    whole table), slack_views, and the whole of every scratch field."""
    stor, seen = {}, set()

    def add(t):
        key = (t.untyped_storage().data_ptr(), tuple(t.shape), tuple(t.stride()), t.storage_offset(), t.element_size())
        if key in seen:
            return
        seen.add(key)
        m = P._byte_mask(t)
        ent = stor.get(key[0])
        if ent is None:
            stor[key[0]] = [t, m]
        else:
            ent[1] |= m

    for op in list(plan.prologue_ops) + list(plan.step_ops) + list(plan.jump_ops) + list(plan.health_ops):
        f = P.fields_of(op)
        if isinstance(op, O.GroupStats):
            add(op.out)
        else:
            for v in P.out_views(op).values():
                add(v)
        for v in P.slack_views(op):
            add(v)
        for k in f.scratch:
            if isinstance(getattr(op, k, None), torch.Tensor):
                add(getattr(op, k))
    return stor


def poison(plan):
    """Fill exactly written_bytes(plan): NaN into floating-point storages, INT_POISON into integer ones.  CPU plans only.  Returns the
    number of bytes filled."""
    assert torch.device(plan.device).type == "cpu", "the byte poison is for the interpreter: a wild counter in front of a kernel is a wild address"
    total = 0
    for t, mask in written_bytes(plan).values():
        es = t.element_size()
        n = t.untyped_storage().nbytes() // es
        whole = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), 0, (n,))
        elems = mask[:n * es].view(n, es).any(1)
        if t.is_floating_point():
            whole[elems] = float("nan")
        else:
            whole[elems] = INT_POISON & ((1 << (8 * es - 1)) - 1) if t.dtype != torch.uint8 else 0x5A
        total += int(elems.sum()) * es
    return total


class NoReset:
    """Stands in for one state tensor of a plan while load_inputs runs: zero_ / copy_ / fill_ do nothing, everything else is the tensor's.
    The seeded omission of tests/test_call_state_*.py: the ops hold the tensor itself, only load_inputs goes through the plan's attribute."""

    def __init__(self, t):
        self.t = t

    def zero_(self):
        return self

    def copy_(self, *a, **k):
        return self

    def fill_(self, *a, **k):
        return self

    def __getattr__(self, name):
        return getattr(self.t, name)

    def __getitem__(self, i):
        return self.t[i]

    def __mul__(self, other):
        return self.t * other

    __rmul__ = __mul__
