"""``VanillaAstar`` / ``NeuralAstar`` -- the drop-in boundary (reference ``planner/astar.py``).

Same constructors, attributes (``astar``, ``encoder``, ``g_ratio``, ``encode``, ``perform_astar``) and state-dict
keys (``astar.neighbor_filter``, ``encoder.model.<n>.*``) as the reference (astar.py:17-46,105-152), so
``scripts/train.py`` and ``utils/training.py`` run unchanged against this package.

Not drop-in (by design): ``use_differentiable_astar=False`` (the reference's CPU ``pq_astar``, a
different algorithm; the reference's own ``tests/astar_test.py::test_pq_astar`` therefore needs the reference package) raises;
CPU tensors raise (no CPU fallback), so ``scripts/create_gif.py``, which never moves the planner or its data to a device, needs
a one-line ``.cuda()`` on both to run.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import encoder
from .differentiable_astar import (AstarOutput, DifferentiableAstar, FieldOutput, FieldRoutesOutput, PathOutput, RoutedAstarOutput,
                                    _checked_heuristic, _checked_route_len)
from .. import ops
from .pq_astar import pq_astar  # noqa: F401  (the reference's astar.py imports it here: a stub that fails loudly when called)


def _is_depth4_cnn(enc: nn.Module) -> bool:
    """The HIP encoder kernels implement the reference's default depth-4 CNN (.. -> 32 -> 64 -> 128 -> 256 -> 1) only; any other
    depth keeps the torch encoder."""
    convs = [m for m in enc.model if isinstance(m, nn.Conv2d)]
    return [c.out_channels for c in convs] == [32, 64, 128, 256, 1] and convs[0].in_channels <= 16


def _downsize_cls():
    from ..encoder_hip import HipCnnDownSizeEncoder
    return HipCnnDownSizeEncoder


class VanillaAstar(nn.Module):
    def __init__(self, g_ratio: float = 0.5, use_differentiable_astar: bool = True):
        """Vanilla A*: cost map = obstacle map = ``map_designs`` (reference astar.py:17-46,93-94).

        Examples:
            >>> planner = VanillaAstar().cuda()
            >>> outputs = planner(map_designs, start_maps, goal_maps)
            >>> outputs.histories, outputs.paths
        """
        super().__init__()
        self.astar = DifferentiableAstar(g_ratio=g_ratio, Tmax=1.0)
        self.g_ratio = g_ratio
        self.use_differentiable_astar = use_differentiable_astar

    @property
    def multi_source(self) -> bool:
        """``self.astar.multi_source``: True = every non-zero cell of ``start_maps`` is a source of the search (``forward()`` and
        ``plan_routes()``); False (default) = the highest-index one only, as before."""
        return self.astar.multi_source

    @multi_source.setter
    def multi_source(self, value: bool) -> None:
        self.astar.multi_source = bool(value)

    def perform_astar(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                      obstacles_maps: torch.Tensor, store_intermediate_results: bool = False,
                      heuristic_maps: Optional[torch.Tensor] = None) -> AstarOutput:
        """``heuristic_maps``: [B,1,H,W] fp32 heuristic in place of the reference's get_heuristic (``DifferentiableAstar.forward``)"""
        if not self.use_differentiable_astar:
            # reference astar.py:57-61 dispatches to pq_astar (CPU numpy + pqdict): a different, non-differentiable
            # algorithm (it charges the NEIGHBOUR's cost, pq_astar.py:138-144) that is outside the hot path.
            raise NotImplementedError(
                "use_differentiable_astar=False selects the reference's CPU-only pq_astar, which is out of scope for "
                "the MI355X-native hot path; the HIP DifferentiableAstar kernel has no large-map penalty, use it.")
        if heuristic_maps is None:
            return self.astar(map_designs, start_maps, goal_maps, obstacles_maps, store_intermediate_results)
        return self.astar(map_designs, start_maps, goal_maps, obstacles_maps, store_intermediate_results, heuristic_maps=heuristic_maps)

    def forward(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                store_intermediate_results: bool = False, heuristic_maps: Optional[torch.Tensor] = None) -> AstarOutput:
        return self.perform_astar(map_designs, start_maps, goal_maps, map_designs, store_intermediate_results, heuristic_maps)


    def plan_routes(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                    heuristic_maps: Optional[torch.Tensor] = None, max_route_len: Optional[int] = None) -> RoutedAstarOutput:
        """``forward()``'s search with every map's ORDERED route, its length and its cost beside the two masks
        (``DifferentiableAstar.plan_routes``): an evaluation call -- no autograd graph, detached tensors."""
        if not self.use_differentiable_astar:
            raise NotImplementedError("use_differentiable_astar=False selects the reference's CPU-only pq_astar, which is out of scope for "
                                      "the MI355X-native hot path; plan_routes() runs the HIP DifferentiableAstar kernel only")
        return self.astar.plan_routes(map_designs, start_maps, goal_maps, map_designs, heuristic_maps, max_route_len)

    def cost_to_go(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, policies: bool = True, tiled: bool = False,
                   differentiable: bool = False) -> FieldOutput:
        """The exact cost to the goal from every cell and the optimal policy (``DifferentiableAstar.cost_to_go``) with cost = passable =
        ``map_designs``: on a binary map the number of moves to the goal.  ``differentiable=True``: ``dists`` carries the gradient to
        ``map_designs`` as the cost (not as the obstacles)."""
        return self.astar.cost_to_go(map_designs, goal_maps, map_designs, policies, tiled, differentiable)

    def cost_to_go_tiled(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, policies: bool = True, differentiable: bool = False) -> FieldOutput:
        """``cost_to_go`` by the tiled relaxation (``DifferentiableAstar.cost_to_go_tiled``: maps of up to 1024x1152, the same bits), with
        cost = passable = ``map_designs``.  ``differentiable=True``: ``dists`` carries the gradient to ``map_designs`` as the cost."""
        return self.astar.cost_to_go_tiled(map_designs, goal_maps, map_designs, policies, differentiable)

    def soft_cost_to_go(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                        policies: bool = False, differentiable: bool = False):
        """The entropy-regularised cost-to-go field over ``horizon`` moves (``DifferentiableAstar.soft_cost_to_go``) with cost = passable =
        ``map_designs``.  ``differentiable=True``: ``dists`` carries the gradient to ``map_designs`` as the cost (not as the obstacles)."""
        return self.astar.soft_cost_to_go(map_designs, goal_maps, map_designs, tau, horizon, policies, differentiable)

    def soft_cost_to_go_tiled(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                              policies: bool = False, differentiable: bool = False, checkpoint_every: Optional[int] = None):
        """``soft_cost_to_go`` by tiled sweeps (``DifferentiableAstar.soft_cost_to_go_tiled``: maps of up to 1024x1152, the same bits)."""
        return self.astar.soft_cost_to_go_tiled(map_designs, goal_maps, map_designs, tau, horizon, policies, differentiable, checkpoint_every)

    def maxent_path_nll(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, opt_trajs: torch.Tensor, tau: float,
                        horizon: Optional[int] = None, tiled: bool = False, checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The maximum-entropy negative log-likelihood [B] of the demonstrations ``opt_trajs`` (``DifferentiableAstar.maxent_path_nll``)
        with cost = passable = ``map_designs``; ``tiled=True`` for maps of up to 1024x1152."""
        return self.astar.maxent_path_nll(map_designs, start_maps, goal_maps, map_designs, opt_trajs, tau, horizon, tiled, checkpoint_every)

    def soft_policy(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, tau: float, horizon: Optional[int] = None):
        """The soft field and the log of its soft policy (``DifferentiableAstar.soft_policy``) with cost = passable = ``map_designs``; both
        carry the gradient to ``map_designs`` as the cost when it requires one."""
        return self.astar.soft_policy(map_designs, goal_maps, map_designs, tau, horizon)

    def soft_policy_tiled(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, tau: float, horizon: Optional[int] = None,
                          checkpoint_every: Optional[int] = None):
        """``soft_policy`` by tiled sweeps (``DifferentiableAstar.soft_policy_tiled``: maps of up to 1024x1152, the same bits)."""
        return self.astar.soft_policy_tiled(map_designs, goal_maps, map_designs, tau, horizon, checkpoint_every)

    def policy_nll(self, map_designs: torch.Tensor, goal_maps: torch.Tensor, opt_policies: torch.Tensor, tau: float,
                   horizon: Optional[int] = None, tiled: bool = False, checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The per-cell imitation loss [B] against the demonstrated actions ``opt_policies`` [B,8,H,W] (``DifferentiableAstar.policy_nll``)
        with cost = passable = ``map_designs``; ``tiled=True`` for maps of up to 1024x1152."""
        return self.astar.policy_nll(map_designs, goal_maps, map_designs, opt_policies, tau, horizon, tiled, checkpoint_every)

    def plan_many(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, max_route_len: Optional[int] = None,
                  paths: bool = False) -> FieldRoutesOutput:
        """The ordered optimal route from each of S start cells per map (``DifferentiableAstar.plan_many``: one field per map, a chase per
        start) with cost = passable = ``map_designs``: on a binary map, shortest routes.  An evaluation call."""
        return self.astar.plan_many(map_designs, starts, goal_maps, map_designs, max_route_len, paths)

    def sample_routes(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float, num_samples: int = 1,
                      seed: Optional[int] = None, horizon: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False):
        """``num_samples`` routes from each of S start cells per map, sampled from the maximum-entropy route distribution
        (``DifferentiableAstar.sample_routes``) with cost = passable = ``map_designs``: on a binary map a route of L moves has weight
        exp(-L / tau).  An evaluation call."""
        return self.astar.sample_routes(map_designs, starts, goal_maps, map_designs, tau, num_samples, seed, horizon, max_route_len, visits)

    def sample_routes_differentiable(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                                     num_samples: int = 1, seed: Optional[int] = None, horizon: Optional[int] = None,
                                     max_route_len: Optional[int] = None, visits: bool = False):
        """``sample_routes`` with ``log_probs`` as a differentiable output (``DifferentiableAstar.sample_routes_differentiable``) with
        cost = passable = ``map_designs``: the score-function gradient goes to ``map_designs`` as the cost when it requires one."""
        return self.astar.sample_routes_differentiable(map_designs, starts, goal_maps, map_designs, tau, num_samples, seed, horizon, max_route_len,
                                                       visits)

    def sample_routes_tiled(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float, num_samples: int = 1,
                            seed: Optional[int] = None, horizon: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False,
                            checkpoint_every: Optional[int] = None):
        """``sample_routes`` from the tiled soft field's checkpointed tape (``DifferentiableAstar.sample_routes_tiled``: maps of up to
        1024x1152, the same bits)."""
        return self.astar.sample_routes_tiled(map_designs, starts, goal_maps, map_designs, tau, num_samples, seed, horizon, max_route_len, visits,
                                              checkpoint_every)

    def shortest_paths(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, lambda_: Optional[float] = None,
                       min_cost: float = 2.0 ** -10) -> PathOutput:
        """The exact optimal path of every map as a 0/1 mask (``DifferentiableAstar.shortest_paths``: field and chase in one launch) with
        cost = passable = ``map_designs``: on a binary map, a shortest route.  ``lambda_``: ``paths`` carries the blackbox gradient to
        ``map_designs`` as the cost (not as the obstacles)."""
        return self.astar.shortest_paths(map_designs, start_maps, goal_maps, map_designs, lambda_, min_cost)

    def shortest_paths_tiled(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, lambda_: Optional[float] = None,
                             min_cost: float = 2.0 ** -10) -> PathOutput:
        """``shortest_paths`` by the tiled relaxation (``DifferentiableAstar.shortest_paths_tiled``: maps of up to 1024x1152, the same bits);
        the call blocks."""
        return self.astar.shortest_paths_tiled(map_designs, start_maps, goal_maps, map_designs, lambda_, min_cost)


class NeuralAstar(VanillaAstar):
    def __init__(self, g_ratio: float = 0.5, Tmax: float = 1.0, encoder_input: str = "m+",
                 encoder_arch: str = "CNN", encoder_depth: int = 4, learn_obstacles: bool = False,
                 const: float = None, use_differentiable_astar: bool = True):
        """Neural A*: an encoder predicts the cost map, then the same search runs (reference astar.py:105-152).

        Args mirror the reference: ``encoder_input`` "m+" = map + (start+goal) channel, "m" = map only;
        ``encoder_arch`` in {"CNN", "CNNDownSize", "Unet"}; ``learn_obstacles`` hides the obstacle map from the search;
        ``const`` = learnable scale on the predicted cost.
        """
        super().__init__()
        self.astar = DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax)
        self.encoder_input = encoder_input
        self.encoder = getattr(encoder, encoder_arch)(len(self.encoder_input), encoder_depth, const)
        self.learn_obstacles = learn_obstacles
        if self.learn_obstacles:
            print("WARNING: learn_obstacles has been set to True")
        self.g_ratio = g_ratio
        self.use_differentiable_astar = use_differentiable_astar
        # Which kernels predict the cost map.  "auto" (default): on a HIP device "hip_f16x3", on CPU tensors "torch" -- decided per
        # call from the input's device, before any BatchNorm state is touched, so that the reference's scripts/train.py:30-50
        # (which constructs NeuralAstar(...) with no such knob) trains and validates on the MFMA kernels unmodified.  "torch" = fp32
        # torch.nn (MIOpen), "hip_bf16" (bf16-MFMA inference kernels for the depth-4 CNN encoder, csrc/nastar_encoder.hip.h),
        # "hip_f16" (plain fp16 operands) or "hip_f16x3" (split fp16 operands: 3x the matrix work, cost maps within 1e-5 of the fp32
        # encoder -- the only hip_* mode that meets the reference's float tolerance, hence what "auto" picks).  With a hip_* backend:
        # eval mode under no_grad = the inference kernels (CNN of any depth / size, CNNDownSize, Unet); training mode with autograd on
        # = the training kernels of neural_astar/encoder_train.py (forward, input and weight gradients, batch-statistics BatchNorm,
        # max-pool, upsample-concat) for CNN of any depth / map size, CNNDownSize and the VggUnet definition of Unet; shapes those
        # kernels do not take, and eval mode with gradients, stay on torch.nn.  Not part of the reference's constructor.
        # "hip_strict" = "hip_f16x3" that RAISES instead of falling back to torch.nn for a shape / mode the kernels do not take.
        self.encoder_backend = "auto"
        self._hip_encoder = None
        # which code predicted the latest cost map: "hip:<kernel family>/<precision>" or "torch.nn" (+ why); a fall-back to torch.nn on a HIP
        # device under a hip_* backend also warns once per reason (a shape that misses must not train on MIOpen without a word)
        self.last_encoder_route: str = ""
        self._route_warned: set = set()

    def effective_encoder_backend(self, like: torch.Tensor) -> str:
        """``encoder_backend`` with "auto" resolved for a tensor on ``like``'s device."""
        if self.encoder_backend == "auto":
            return "hip_f16x3" if like.is_cuda else "torch"
        if self.encoder_backend == "hip_strict":
            return "hip_f16x3"
        return self.encoder_backend

    def _routed(self, route: str, cost: torch.Tensor) -> torch.Tensor:
        self.last_encoder_route = route
        return cost

    def encode(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor) -> torch.Tensor:
        """Predict cost maps (reference astar.py:154-180)."""
        backend = self.effective_encoder_backend(map_designs)
        if (backend.startswith("hip") and not self.training and not torch.is_grad_enabled()
                and isinstance(self.encoder, encoder.CNNDownSize)):
            # CNNDownSize (WarCraft): f32-input MFMA kernels at fp32 accuracy whatever the hip_* precision asked for
            convs = [m for m in self.encoder.model if isinstance(m, nn.Conv2d)]
            depth = len(convs) - 1
            plus = "+" in self.encoder_input
            if (1 <= depth <= 4 and [c.out_channels for c in convs] == [32, 64, 128, 256][:depth] + [1] and convs[0].in_channels <= 4
                    and map_designs.shape[1] + int(plus) == convs[0].in_channels
                    and map_designs.shape[-2] % (1 << depth) == 0 and map_designs.shape[-1] % (1 << depth) == 0):
                if not isinstance(self._hip_encoder, _downsize_cls()):
                    self._hip_encoder = _downsize_cls()(self.encoder)
                return self._routed("hip:CNNDownSize-infer/f32", self._hip_encoder(map_designs, start_maps, goal_maps, plus))
        if (backend.startswith("hip") and not self.training and not torch.is_grad_enabled()
                and isinstance(self.encoder, encoder.Unet) and isinstance(self.encoder.model, encoder.VggUnet)
                and map_designs.shape[1] == 1 and map_designs.shape[-2:] == start_maps.shape[-2:]
                and map_designs.shape[-2] % (1 << self.encoder.model.depth) == 0
                and map_designs.shape[-1] % (1 << self.encoder.model.depth) == 0):
            # Unet(vgg16_bn): generic fp16 MFMA convolution (csrc/nastar_conv_flat.hip.h); "hip_f16x3" = split operands, fp32-grade
            precision = "f16x3" if backend == "hip_f16x3" else "f16"
            from ..encoder_hip import HipUnetEncoder
            if type(self._hip_encoder) is not HipUnetEncoder or self._hip_encoder.precision != precision:
                self._hip_encoder = HipUnetEncoder(self.encoder, precision)
            return self._routed(f"hip:Unet-infer/{precision}", self._hip_encoder(map_designs, start_maps, goal_maps, "+" in self.encoder_input))
        # (training mode under no_grad -- a validation pass somebody forgot to switch to eval() -- is the same forward: batch statistics, running
        #  statistics updated; the autograd functions then simply record nothing)
        if (backend.startswith("hip") and map_designs.is_cuda
                and (self.encoder.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.encoder.parameters())))
                and isinstance(self.encoder, encoder.Unet) and map_designs.shape[1] == 1
                and map_designs.shape[-2:] == start_maps.shape[-2:]):
            from ..encoder_train import unet_supported, unet_train_forward
            first = next(m for m in self.encoder.model.modules() if isinstance(m, nn.Conv2d))
            if (unet_supported(self.encoder, map_designs.shape[-2], map_designs.shape[-1])
                    and first.in_channels == 1 + int("+" in self.encoder_input)):
                prec = "f16" if backend == "hip_f16" else "f16x3"
                return self._routed(f"hip:Unet-{'train' if self.encoder.training else 'evalgrad'}/{prec}", unet_train_forward(self.encoder, map_designs, start_maps, goal_maps,
                                                                                 "+" in self.encoder_input, prec))
        if (backend.startswith("hip") and map_designs.is_cuda and isinstance(self.encoder, encoder.CNN)
                and (self.encoder.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.encoder.parameters())))):
            # UNDER AUTOGRAD: convolutions, BatchNorm (batch statistics in training mode; the running statistics in eval mode -- round 6),
            # ReLU, max-pool and all their gradients on the MI355X kernels (neural_astar/encoder_train.py); "hip_f16" = plain fp16
            # operands, anything else = split operands (fp32-grade).  CNN (any depth) and CNNDownSize (WarCraft); shapes the kernels do
            # not take stay on torch.nn.
            from ..encoder_train import cnn_train_forward, supported
            convs = [m for m in self.encoder.model if isinstance(m, nn.Conv2d)]
            pool = isinstance(self.encoder, encoder.CNNDownSize)
            plus = "+" in self.encoder_input
            if (supported(self.encoder, map_designs.shape[-2], map_designs.shape[-1])
                    and map_designs.shape[1] + int(plus) == convs[0].in_channels
                    and (pool or map_designs.shape[-2:] == start_maps.shape[-2:])):
                prec = "f16" if backend == "hip_f16" else "f16x3"
                kind = "train" if self.encoder.training else "evalgrad"
                return self._routed(f"hip:{'CNNDownSize' if pool else 'CNN'}-{kind}/{prec}",
                                    cnn_train_forward(self.encoder, map_designs, start_maps, goal_maps, plus, prec))
        tile = 32 if backend in ("hip_f16", "hip_f16x3") else 16
        if (backend in ("hip_bf16", "hip_f16", "hip_f16x3") and not self.training and not torch.is_grad_enabled()
                and map_designs.shape[1] == 1 and map_designs.shape[-2:] == start_maps.shape[-2:]
                and map_designs.shape[-2] % tile == 0 and map_designs.shape[-1] % 32 == 0
                and isinstance(self.encoder, encoder.CNN) and not isinstance(self.encoder, encoder.CNNDownSize)
                and _is_depth4_cnn(self.encoder)):
            precision = backend[4:]
            from ..encoder_hip import HipCnnEncoder
            if type(self._hip_encoder) is not HipCnnEncoder or self._hip_encoder.precision != precision:
                self._hip_encoder = HipCnnEncoder(self.encoder, precision)
            return self._routed(f"hip:CNN-infer-img32/{precision}", self._hip_encoder(map_designs, start_maps, goal_maps, "+" in self.encoder_input))
        if (backend.startswith("hip") and not self.training and not torch.is_grad_enabled()
                and type(self.encoder) is encoder.CNN and map_designs.shape[1] == 1 and map_designs.shape[-2:] == start_maps.shape[-2:]
                and self.encoder.model[0].in_channels == 1 + int("+" in self.encoder_input)):
            # any other depth / map size: the generic fp16 MFMA convolution ("hip_f16x3" = split operands, otherwise plain fp16)
            precision = "f16x3" if backend == "hip_f16x3" else "f16"
            from ..encoder_hip import HipFlatCnnEncoder
            if type(self._hip_encoder) is not HipFlatCnnEncoder or self._hip_encoder.precision != precision:
                self._hip_encoder = HipFlatCnnEncoder(self.encoder, precision)
            return self._routed(f"hip:CNN-infer-flat/{precision}", self._hip_encoder(map_designs, start_maps, goal_maps, "+" in self.encoder_input))
        # torch.nn (MIOpen on a HIP device): the CPU path, the "torch" backend -- or a shape / mode the kernels do not take
        route = "torch.nn"
        if backend.startswith("hip"):
            why = (f"{type(self.encoder).__name__} on {tuple(map_designs.shape)} maps, training={self.encoder.training}, "
                   f"grad={torch.is_grad_enabled()}, device={map_designs.device.type}")
            route = f"torch.nn (fell through from {backend}: {why})"
            if self.encoder_backend == "hip_strict":
                raise RuntimeError(f"encoder_backend='hip_strict': no MI355X encoder kernel takes {why}; it would run on torch.nn")
            if map_designs.is_cuda and why not in self._route_warned:
                self._route_warned.add(why)
                import warnings
                warnings.warn(f"NeuralAstar.encode: {why} is not covered by the MI355X encoder kernels -- this call runs on torch.nn (MIOpen); "
                              "planner.last_encoder_route records the route, encoder_backend='hip_strict' turns this into an error, "
                              "'torch' silences it", RuntimeWarning, stacklevel=2)
        self.last_encoder_route = route
        inputs = map_designs
        if "+" in self.encoder_input:
            sg = start_maps + goal_maps
            if map_designs.shape[-1] != start_maps.shape[-1]:  # WarCraft: 96x96 image vs 12x12 grid
                sg = nn.functional.interpolate(sg, size=map_designs.shape[-2:], mode="nearest")
            inputs = torch.cat((inputs, sg), dim=1)
        return self.encoder(inputs)

    def forward(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                store_intermediate_results: bool = False, heuristic_maps: Optional[torch.Tensor] = None) -> AstarOutput:
        cost_maps = self.encode(map_designs, start_maps, goal_maps)
        obstacles_maps = map_designs if not self.learn_obstacles else torch.ones_like(start_maps)
        return self.perform_astar(cost_maps, start_maps, goal_maps, obstacles_maps, store_intermediate_results, heuristic_maps)

    def plan_routes(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor,
                    heuristic_maps: Optional[torch.Tensor] = None, max_route_len: Optional[int] = None) -> RoutedAstarOutput:
        """``forward()``'s encode + search with every map's ORDERED route, its length and its cost beside the two masks
        (``DifferentiableAstar.plan_routes``): an evaluation call -- the predicted cost maps are detached, no autograd graph is kept."""
        _checked_route_len(max_route_len)  # (both refusals before the encoder launches anything)
        if heuristic_maps is not None:
            _checked_heuristic(heuristic_maps, start_maps)
        if not self.use_differentiable_astar:
            raise NotImplementedError("use_differentiable_astar=False selects the reference's CPU-only pq_astar, which is out of scope for "
                                      "the MI355X-native hot path; plan_routes() runs the HIP DifferentiableAstar kernel only")
        cost_maps = self.encode(map_designs, start_maps, goal_maps).detach()
        obstacles_maps = map_designs if not self.learn_obstacles else torch.ones_like(start_maps)
        return self.astar.plan_routes(cost_maps, start_maps, goal_maps, obstacles_maps, heuristic_maps, max_route_len)

    def _field_inputs(self, map_designs, start_maps, goal_maps, detach: bool):
        """``(cost_maps, obstacles_maps)`` of a field call: the PREDICTED cost maps -- ``detach``: cut from the encoder -- and the obstacles
        the search would see (``learn_obstacles``: every cell passable)"""
        cost_maps = self.encode(map_designs, start_maps, goal_maps)
        obstacles_maps = map_designs if not self.learn_obstacles else torch.ones_like(start_maps)
        return (cost_maps.detach() if detach else cost_maps), obstacles_maps

    def cost_to_go(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, policies: bool = True,
                   tiled: bool = False, differentiable: bool = False) -> FieldOutput:
        """The cost-to-go field and optimal policy of the PREDICTED cost maps: encodes as ``plan_routes()`` does (detached), then
        ``DifferentiableAstar.cost_to_go``; ``learn_obstacles`` makes every cell passable, as it does for the search.
        ``differentiable=True``: the encoded cost maps are NOT detached, so the gradient of ``dists`` reaches the encoder's parameters
        (value-function supervision; the loss masks the +inf cells itself).  The encoder route is what ``encode()`` picks in that mode."""
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=not differentiable)
        return self.astar.cost_to_go(cost_maps, goal_maps, obstacles_maps, policies, tiled, differentiable)

    def cost_to_go_tiled(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, policies: bool = True,
                         differentiable: bool = False) -> FieldOutput:
        """``cost_to_go`` of the PREDICTED cost maps by the tiled relaxation (maps of up to 1024x1152; the call blocks).
        ``differentiable=True``: the encoded cost maps are NOT detached, exactly as in ``cost_to_go``, so a loss on ``dists`` trains the
        encoder on maps of any size the search takes (include/nastar_fields_grad_tiled.h)."""
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=not differentiable)
        return self.astar.cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, policies, differentiable)

    def soft_cost_to_go(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                        horizon: Optional[int] = None, policies: bool = False, differentiable: bool = False):
        """The entropy-regularised cost-to-go field of the PREDICTED cost maps: encodes as ``cost_to_go()`` does (detached unless
        ``differentiable``), then ``DifferentiableAstar.soft_cost_to_go``; ``learn_obstacles`` makes every cell passable."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=not differentiable)
        return self.astar.soft_cost_to_go(cost_maps, goal_maps, obstacles_maps, tau, horizon, policies, differentiable)

    def soft_cost_to_go_tiled(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                              horizon: Optional[int] = None, policies: bool = False, differentiable: bool = False,
                              checkpoint_every: Optional[int] = None):
        """``soft_cost_to_go`` of the PREDICTED cost maps by tiled sweeps (``DifferentiableAstar.soft_cost_to_go_tiled``: maps of up to
        1024x1152, the same bits)."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=not differentiable)
        return self.astar.soft_cost_to_go_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, policies, differentiable, checkpoint_every)

    def maxent_path_nll(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, opt_trajs: torch.Tensor,
                        tau: float, horizon: Optional[int] = None, tiled: bool = False, checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The maximum-entropy IRL loss of the demonstrations ``opt_trajs`` under the PREDICTED cost maps -> [B]
        (``ops.maxent_path_nll``): encodes as ``forward()`` does, NOT detached, so ``.sum().backward()`` trains the encoder with the
        gradient (demonstration - expected visits) / tau; ``learn_obstacles`` makes every cell passable.  ``tiled=True``: on the tiled
        field (maps of up to 1024x1152), with its ``checkpoint_every``."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=False)
        return self.astar.maxent_path_nll(cost_maps, start_maps, goal_maps, obstacles_maps, opt_trajs, tau, horizon, tiled, checkpoint_every)

    def soft_policy(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                    horizon: Optional[int] = None):
        """The soft field of the PREDICTED cost maps and the log of its soft policy (``ops.soft_policy``): encodes as ``forward()`` does,
        NOT detached, so a loss on ``dists`` or ``log_policies`` trains the encoder (no graph under ``torch.no_grad()``);
        ``learn_obstacles`` makes every cell passable."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=False)
        return self.astar.soft_policy(cost_maps, goal_maps, obstacles_maps, tau, horizon)

    def soft_policy_tiled(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                          horizon: Optional[int] = None, checkpoint_every: Optional[int] = None):
        """``soft_policy`` of the PREDICTED cost maps by tiled sweeps (``DifferentiableAstar.soft_policy_tiled``: maps of up to 1024x1152,
        the same bits): encodes as ``soft_policy`` does, NOT detached."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=False)
        return self.astar.soft_policy_tiled(cost_maps, goal_maps, obstacles_maps, tau, horizon, checkpoint_every)

    def policy_nll(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, opt_policies: torch.Tensor,
                   tau: float, horizon: Optional[int] = None, tiled: bool = False, checkpoint_every: Optional[int] = None) -> torch.Tensor:
        """The per-cell imitation loss of the demonstrated actions ``opt_policies`` [B,8,H,W] under the PREDICTED cost maps -> [B]
        (``ops.soft_policy_nll``): the cross-entropy between the soft policy and the optimal action of every cell, thousands of
        supervised cells per map.  Encodes as ``forward()`` does, NOT detached, so ``.sum().backward()`` trains the encoder;
        ``learn_obstacles`` makes every cell passable.  ``tiled=True``: on the tiled policy (maps of up to 1024x1152), with its
        ``checkpoint_every``."""
        ops._checked_tau(tau)  # (before the encoder launches anything)
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=False)
        return self.astar.policy_nll(cost_maps, goal_maps, obstacles_maps, opt_policies, tau, horizon, tiled, checkpoint_every)

    def plan_many(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, max_route_len: Optional[int] = None,
                  paths: bool = False) -> FieldRoutesOutput:
        """The ordered optimal route, under the PREDICTED cost maps, from each of S start cells per map (``DifferentiableAstar.plan_many``).
        For ``encoder_input == "m"`` only: the maps are encoded once (detached, with an all-zero start channel) and one field serves every
        start.  With "m+" the cost map depends on the start, so one field cannot serve S starts: NotImplementedError.  An evaluation
        call; ``learn_obstacles`` makes every cell passable, as it does for the search."""
        _checked_route_len(max_route_len)  # (both refusals before the encoder launches anything)
        if self.encoder_input != "m":
            raise NotImplementedError(f"NeuralAstar.plan_many: with encoder_input={self.encoder_input!r} the predicted cost map depends on the "
                                      "start, so one cost-to-go field cannot serve several starts; encode per start and call "
                                      "planner.astar.plan_many(cost_maps, starts, goal_maps, obstacles_maps), or use encoder_input='m'")
        cost_maps = self.encode(map_designs, torch.zeros_like(goal_maps), goal_maps).detach()
        obstacles_maps = map_designs if not self.learn_obstacles else torch.ones_like(goal_maps)
        return self.astar.plan_many(cost_maps, starts, goal_maps, obstacles_maps, max_route_len, paths)

    def sample_routes(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float, num_samples: int = 1,
                      seed: Optional[int] = None, horizon: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False):
        """``num_samples`` routes from each of S start cells per map, sampled from the maximum-entropy route distribution of the PREDICTED
        cost maps (``DifferentiableAstar.sample_routes``): what a model trained with ``maxent_path_nll`` generates.  For
        ``encoder_input == "m"`` only, as ``plan_many``: the maps are encoded once (detached, with an all-zero start channel) and one soft
        field serves every start; with "m+" NotImplementedError.  An evaluation call; ``learn_obstacles`` makes every cell passable."""
        _checked_route_len(max_route_len)  # (every refusal before the encoder launches anything)
        ops._checked_tau(tau)
        ops._checked_samples(num_samples)
        if self.encoder_input != "m":
            raise NotImplementedError(f"NeuralAstar.sample_routes: with encoder_input={self.encoder_input!r} the predicted cost map depends on "
                                      "the start, so one soft field cannot serve several starts; encode per start and call "
                                      "planner.astar.sample_routes(cost_maps, starts, goal_maps, obstacles_maps, tau), or use encoder_input='m'")
        return self.astar.sample_routes(*self._sample_inputs(map_designs, starts, goal_maps), tau, num_samples, seed, horizon, max_route_len, visits)

    def sample_routes_differentiable(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float,
                                     num_samples: int = 1, seed: Optional[int] = None, horizon: Optional[int] = None,
                                     max_route_len: Optional[int] = None, visits: bool = False):
        """``sample_routes`` on the PREDICTED cost maps with ``log_probs`` as a differentiable output
        (``DifferentiableAstar.sample_routes_differentiable``): encodes as ``sample_routes`` does -- once, with an all-zero start channel,
        ``encoder_input == "m"`` only -- but NOT detached, so ``ops.route_score_loss(out.log_probs, rewards, out.status).backward()``
        trains the encoder on any reward per sampled route (REINFORCE); no graph under ``torch.no_grad()``."""
        _checked_route_len(max_route_len)  # (every refusal before the encoder launches anything)
        ops._checked_tau(tau)
        ops._checked_samples(num_samples)
        if self.encoder_input != "m":
            raise NotImplementedError(f"NeuralAstar.sample_routes_differentiable: with encoder_input={self.encoder_input!r} the predicted cost "
                                      "map depends on the start, so one soft field cannot serve several starts; encode per start and call "
                                      "planner.astar.sample_routes_differentiable(cost_maps, starts, goal_maps, obstacles_maps, tau), or use "
                                      "encoder_input='m'")
        return self.astar.sample_routes_differentiable(*self._sample_inputs(map_designs, starts, goal_maps, detach=False), tau, num_samples, seed,
                                                       horizon, max_route_len, visits)

    def sample_routes_tiled(self, map_designs: torch.Tensor, starts: torch.Tensor, goal_maps: torch.Tensor, tau: float, num_samples: int = 1,
                            seed: Optional[int] = None, horizon: Optional[int] = None, max_route_len: Optional[int] = None, visits: bool = False,
                            checkpoint_every: Optional[int] = None):
        """``sample_routes`` on the PREDICTED cost maps from the tiled soft field's checkpointed tape
        (``DifferentiableAstar.sample_routes_tiled``: maps of up to 1024x1152, the same bits): what a model trained with
        ``maxent_path_nll(..., tiled=True)`` generates.  For ``encoder_input == "m"`` only, as ``sample_routes``."""
        _checked_route_len(max_route_len)  # (every refusal before the encoder launches anything)
        ops._checked_tau(tau)
        ops._checked_samples(num_samples)
        if self.encoder_input != "m":
            raise NotImplementedError(f"NeuralAstar.sample_routes_tiled: with encoder_input={self.encoder_input!r} the predicted cost map depends "
                                      "on the start, so one soft field cannot serve several starts; encode per start and call "
                                      "planner.astar.sample_routes_tiled(cost_maps, starts, goal_maps, obstacles_maps, tau), or use "
                                      "encoder_input='m'")
        return self.astar.sample_routes_tiled(*self._sample_inputs(map_designs, starts, goal_maps), tau, num_samples, seed, horizon, max_route_len,
                                              visits, checkpoint_every)

    def _sample_inputs(self, map_designs, starts, goal_maps, detach: bool = True):
        """the (cost, starts, goal, obstacles) maps of ``sample_routes`` and its siblings: encoded once, with an all-zero start channel;
        detached unless the samples' ``log_probs`` are to train the encoder"""
        cost_maps = self.encode(map_designs, torch.zeros_like(goal_maps), goal_maps)
        if detach:
            cost_maps = cost_maps.detach()
        obstacles_maps = map_designs if not self.learn_obstacles else torch.ones_like(goal_maps)
        return cost_maps, starts, goal_maps, obstacles_maps

    def shortest_paths(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, lambda_: Optional[float] = None,
                       min_cost: float = 2.0 ** -10) -> PathOutput:
        """The exact optimal path under the PREDICTED cost maps as a 0/1 mask (``DifferentiableAstar.shortest_paths``): encodes as
        ``forward()`` does, then one launch solves every map; ``learn_obstacles`` makes every cell passable, as it does for the search.
        ``lambda_=None``: an evaluation call on the detached cost maps.  ``lambda_`` a positive float: the cost maps are NOT detached and
        ``paths`` carries the blackbox gradient, so a Hamming or L1 loss on ``paths`` against the demonstration trains the encoder on the
        device (the "BB-A*" baseline of the Neural A* paper).  The encoder route is what ``encode()`` picks in that mode."""
        return self.astar.shortest_paths(*self._path_inputs(map_designs, start_maps, goal_maps, lambda_, min_cost), lambda_, min_cost)

    def shortest_paths_tiled(self, map_designs: torch.Tensor, start_maps: torch.Tensor, goal_maps: torch.Tensor, lambda_: Optional[float] = None,
                             min_cost: float = 2.0 ** -10) -> PathOutput:
        """``shortest_paths`` under the PREDICTED cost maps by the tiled relaxation (``DifferentiableAstar.shortest_paths_tiled``: maps of
        up to 1024x1152, the same bits; the call blocks, and so does its backward).  With ``lambda_`` the cost maps are NOT detached: a loss
        on ``paths`` trains the encoder on maps of any size the search takes (include/nastar_path_masks_tiled.h)."""
        return self.astar.shortest_paths_tiled(*self._path_inputs(map_designs, start_maps, goal_maps, lambda_, min_cost), lambda_, min_cost)

    def _path_inputs(self, map_designs, start_maps, goal_maps, lambda_, min_cost):
        """the (cost, start, goal, obstacles) maps of ``shortest_paths`` / ``shortest_paths_tiled``"""
        if lambda_ is not None:
            ops._checked_step(lambda_, "lambda_")  # (both refusals before the encoder launches anything)
        ops._checked_step(min_cost, "min_cost")
        cost_maps, obstacles_maps = self._field_inputs(map_designs, start_maps, goal_maps, detach=lambda_ is None)
        return cost_maps, start_maps, goal_maps, obstacles_maps
