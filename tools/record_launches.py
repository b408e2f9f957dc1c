#!/usr/bin/env python3
"""Which C-ABI search / replay calls the Python launch layer issues, with which arguments (run on the GPU box): a fixed list of planner and
op calls is driven through a recorder around the loaded library; every pointer argument is printed as the NAME of the tensor it points into
(None = NULL, "<temporary>" = memory the launch layer allocated itself: workspaces, gradients), integers and floats as they are.  One JSON
line per call on stdout.  Two checkouts that print the same lines hand the kernels the same arguments: the check of a change to ops.py /
_native.py that must not change behaviour (profiles/launch_layer/).  The Python host lane is forced (NASTAR_FASTLANE=0)."""
import ctypes
import json
import os
import sys

os.environ["NASTAR_FASTLANE"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "neural-astar_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_astar import _native, ops  # noqa: E402
from neural_astar.parallel import InFlightPlanner  # noqa: E402
from neural_astar.planner import VanillaAstar  # noqa: E402
from neural_astar.planner.differentiable_astar import DifferentiableAstar  # noqa: E402
from neural_astar.utils import synthetic as syn  # noqa: E402

dev = torch.device("cuda:0")
RECORDED = ("nastar_forward", "nastar_backward_replay", "nastar_backward_l1_replay", "nastar_l1_loss", "nastar_placement_from_levels")


class Recorder:
    """stands where ``_native.load()`` keeps the library: calls of the RECORDED entry points are noted, then made"""

    def __init__(self, lib):
        self.lib, self.calls, self.names, self.streams = lib, [], {}, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith(RECORDED):
            return fn

        def call(*args):
            self.calls.append((name, fn.argtypes, args))
            return fn(*args)
        self.__dict__[name] = call
        return call

    def _name(self, ptr):
        if not ptr:
            return None
        for name, t in self.names.items():
            off = ptr - t.data_ptr()
            if 0 <= off < max(t.numel() * t.element_size(), 1):
                return name if off == 0 else f"{name}+{off}"
        board = ops.StatusBoard.of(dev)
        if 0 <= ptr - board.base < board.t.numel() * 4:
            return f"status_summary[{(ptr - board.base) // (4 * ops.SUMMARY_WORDS)}]"
        if 0 <= ptr - board.cbase < board.counters.numel() * 4:
            return f"completion_counter[{(ptr - board.cbase) // 4}]"
        if ptr == torch.cuda.current_stream(dev).cuda_stream:
            return "current stream"
        return self.streams.get(ptr, "<temporary>")

    def flush(self, scenario, **tensors):
        """print the calls noted since the last flush; ``tensors``: what the calls returned, named like the inputs"""
        self.names.update({k: t for k, t in tensors.items() if t is not None})
        for name, argtypes, args in self.calls:
            shown = [self._name(a) if k in (ctypes.c_void_p,) else a for k, a in zip(argtypes, args)]
            print(json.dumps({"scenario": scenario, "symbol": name, "args": shown}), flush=True)
        self.calls = []
        for k in tensors:
            self.names.pop(k, None)


def main():
    rec = _native._lib = Recorder(_native.load())

    def batch(B, H, seed, density=0.2):
        pr = syn.random_obstacle_maps(B, H, H, density, seed=seed)
        m, s, g = (torch.from_numpy(x).to(dev) for x in (pr.map_designs, pr.start_maps, pr.goal_maps))
        cost = torch.from_numpy(syn.random_costs(B, H, H, seed=seed + 1)).to(dev)
        rec.names = {"maps": m, "start": s, "goal": g, "cost": cost}
        return m, s, g, cost

    def planner_call(scenario, astar, cost, s, g, m, grad=False, **kw):
        """one forward() -- and, with ``grad``, the backward of sum(histories * upstream)"""
        if grad:
            cost = cost.detach().requires_grad_(True)
            rec.names["cost"] = cost
        with torch.enable_grad() if grad else torch.no_grad():
            out = astar(cost, s, g, m, **kw)
        rec.flush(scenario, histories=out.histories, paths=out.paths, iters=astar.last_iters, status=astar.last_status)
        if grad:
            up = torch.ones_like(out.histories)
            rec.names["upstream"] = up
            (out.histories * up).sum().backward()
            rec.flush(scenario + " backward", histories=out.histories, iters=astar.last_iters)
        torch.cuda.synchronize()

    m, s, g, cost = batch(64, 32, 11)
    va = VanillaAstar().to(dev).eval()
    with torch.no_grad():
        out = va(m, s, g)
    rec.flush("default no-grad", histories=out.histories, paths=out.paths, iters=va.astar.last_iters, status=va.astar.last_status)
    planner_call("store_intermediate_results", DifferentiableAstar().to(dev).eval(), cost, s, g, m, store_intermediate_results=True)
    da = DifferentiableAstar().to(dev).eval()
    da.check_solvable = "deferred"
    planner_call("check_solvable deferred", da, cost, s, g, m)
    da.raise_if_unsolvable()
    planner_call("autograd, B below PLACEMENT_MIN_BATCH", DifferentiableAstar().to(dev).eval(), cost, s, g, m, grad=True)
    vn = DifferentiableAstar().to(dev).eval()
    with torch.no_grad():
        vn.neighbor_filter.copy_(torch.tensor([[0., 1., 0.], [1., 0., 1.], [0., 1., 0.]]).reshape(1, 1, 3, 3))
    vn.check_solvable = False  # (4-connected: some maps of the batch have no route)
    planner_call("neighbor_filter von Neumann", vn, cost, s, g, m)
    planner_call("neighbor_filter von Neumann, autograd", vn, cost, s, g, m, grad=True)
    h0 = torch.zeros_like(cost)
    rec.names["heuristic"] = h0
    planner_call("heuristic_maps", DifferentiableAstar().to(dev).eval(), cost, s, g, m, heuristic_maps=h0)
    planner_call("heuristic_maps, autograd", DifferentiableAstar().to(dev).eval(), cost, s, g, m, grad=True, heuristic_maps=h0)
    planner_call("g_ratio 0.2", DifferentiableAstar(g_ratio=0.2).to(dev).eval(), cost, s, g, m)
    planner_call("g_ratio 0.2, autograd", DifferentiableAstar(g_ratio=0.2).to(dev).eval(), cost, s, g, m, grad=True)

    m, s, g, cost = batch(ops.PLACEMENT_MIN_BATCH, 32, 21)
    planner_call("autograd, B at PLACEMENT_MIN_BATCH", DifferentiableAstar(Tmax=0.25).to(dev).train(), cost, s, g, m, grad=True)
    lv = torch.arange(ops.PLACEMENT_MIN_BATCH, dtype=torch.int32, device=dev)
    rec.names["levels"] = lv
    ops.attach_order(s, lv)
    rec.names["order"] = s.placement_order.order
    planner_call("loader's order hint", DifferentiableAstar().to(dev).eval(), cost, s, g, m)
    for name, B in (("fused L1 step", 8), ("fused L1 step, B at PLACEMENT_MIN_BATCH", ops.PLACEMENT_MIN_BATCH)):
        c = cost[:B, 0].detach().requires_grad_(True)
        traj = torch.zeros_like(c)
        rec.names.update(cost=c, opt_trajs=traj)
        loss, hist, paths, iters, status = ops.astar_l1_loss(c, s[:B, 0], g[:B, 0], m[:B, 0], traj, 0.5, 256)
        rec.flush(name, histories=hist, paths=paths, iters=iters, status=status, loss=loss)
        loss.backward()
        rec.flush(name + " backward", histories=hist, iters=iters, grad_cost=c.grad)
        torch.cuda.synchronize()

    m, s, g, cost = batch(2, 96, 31)
    planner_call("map above 80x80", DifferentiableAstar().to(dev).eval(), cost, s, g, m)
    planner_call("map above 80x80, autograd", DifferentiableAstar().to(dev).eval(), cost, s, g, m, grad=True)

    m, s, g, cost = batch(64, 32, 41)
    m2 = m.clone()
    m2[3, 0, 9, 9] = 0.5  # not binary: the optimistic unit-cost launch is run again at collection
    rec.names["maps2"] = m2
    fly = InFlightPlanner(VanillaAstar().to(dev).eval(), streams=2)
    fly._setup(dev)
    rec.streams = {p: f"stream {k}" for k, p in enumerate(fly._ptrs)}
    fly.submit(m, s, g)
    fly.submit(m2, s, g)
    rec.flush("InFlightPlanner.submit")
    try:
        outs = fly.collect()
        rec.flush("InFlightPlanner.collect", histories=outs[1].histories, paths=outs[1].paths)
    except Exception as e:  # noqa: BLE001 -- (the edited map may have lost its route: the calls are what is recorded)
        rec.flush("InFlightPlanner.collect")
        print(json.dumps({"scenario": "InFlightPlanner.collect", "raised": type(e).__name__}), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    np.random.seed(0)
    main()
