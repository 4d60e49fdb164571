"""A stand-in for ``teaserpp_python`` with the names registration_node.py:112-131 uses, on the GPU (csrc/teaser.hip) with the two
sequential stages on the host inside the library (csrc/teaser_host.cpp).  DESIGN.md 7.8 is the specification: the algorithm is restated
with every tie and every order of summation decided, and parity with the library itself is not pinned (it is not a dependency).

    params = RobustRegistrationSolver.Params()          # the fields of RN:113-124
    solver = RobustRegistrationSolver(params)
    solver.solve(src, dst)                               # 3 x N arrays (numpy, or fp64 tensors on the device)
    solution = solver.getSolution()                      # .rotation, .translation, .scale (1.0), .valid

What the reference's call does not use -- scale estimation, PMC_HEU and the other inlier selections, the COMPLETE graph, FGR and Quatro
-- raises NotImplementedError naming it.

A solve makes THREE read-backs, whatever N is: {h, number kept} after the reduction; the kept vertices and their sub-matrix for the
host's search; the rotation, weights, iteration count and the rows ``tgt - R src`` after GNC-TLS."""
from __future__ import annotations

import enum
import math

import numpy as np
import torch

from . import ops


class RegistrationSolution:
    def __init__(self):
        self.valid = False
        self.scale = 1.0
        self.rotation = np.eye(3)
        self.translation = np.zeros(3)


class RobustRegistrationSolver:
    class ROTATION_ESTIMATION_ALGORITHM(enum.Enum):
        GNC_TLS = 0
        FGR = 1
        QUATRO = 2

    class INLIER_GRAPH_FORMULATION(enum.Enum):
        CHAIN = 0
        COMPLETE = 1

    class INLIER_SELECTION_MODE(enum.Enum):
        PMC_EXACT = 0
        PMC_HEU = 1
        KCORE_HEU = 2
        NONE = 3

    class Params:
        """teaser::RobustRegistrationSolver::Params with the library's defaults; RN:113-124 sets every field it relies on."""

        def __init__(self):
            self.noise_bound = 0.01
            self.cbar2 = 1.0
            self.estimate_scaling = True
            self.rotation_estimation_algorithm = RobustRegistrationSolver.ROTATION_ESTIMATION_ALGORITHM.GNC_TLS
            self.rotation_gnc_factor = 1.4
            self.rotation_max_iterations = 100
            self.rotation_cost_threshold = 1e-6
            self.rotation_tim_graph = RobustRegistrationSolver.INLIER_GRAPH_FORMULATION.CHAIN
            self.inlier_selection_mode = RobustRegistrationSolver.INLIER_SELECTION_MODE.PMC_EXACT
            self.kcore_heuristic_threshold = 0.5
            self.use_max_clique = True
            self.max_clique_exact_solution = True
            self.max_clique_time_limit = 3600

    def __init__(self, params: "RobustRegistrationSolver.Params"):
        S = RobustRegistrationSolver
        if params.estimate_scaling:
            raise NotImplementedError("estimate_scaling=True is outside the reference's call (registration_node.py:115)")
        if params.inlier_selection_mode is not S.INLIER_SELECTION_MODE.PMC_EXACT:
            raise NotImplementedError(f"inlier_selection_mode {getattr(params.inlier_selection_mode, 'name', params.inlier_selection_mode)}: "
                                      "only PMC_EXACT is implemented (registration_node.py:116-117)")
        if params.rotation_tim_graph is not S.INLIER_GRAPH_FORMULATION.CHAIN:
            raise NotImplementedError(f"rotation_tim_graph {getattr(params.rotation_tim_graph, 'name', params.rotation_tim_graph)}: "
                                      "only CHAIN is implemented (registration_node.py:118-119)")
        if params.rotation_estimation_algorithm is not S.ROTATION_ESTIMATION_ALGORITHM.GNC_TLS:
            raise NotImplementedError(f"rotation_estimation_algorithm {getattr(params.rotation_estimation_algorithm, 'name', params.rotation_estimation_algorithm)}: "
                                      "only GNC_TLS is implemented (registration_node.py:120-121)")
        if not (params.use_max_clique and params.max_clique_exact_solution):
            raise NotImplementedError("use_max_clique=False / max_clique_exact_solution=False are outside the reference's call")
        if not (0.0 < params.noise_bound < math.inf and 0.0 < params.cbar2 < math.inf):
            raise ValueError("noise_bound and cbar2 must be positive and finite")
        self.params = params
        self.node_limit = ops.TEASER_NODE_LIMIT
        self.reset(params)

    def reset(self, params=None):
        if params is not None:
            self.params = params
        self._solution = RegistrationSolution()
        self._clique = np.zeros(0, dtype=np.int32)
        self._weights = np.zeros(0)
        self._translation_inliers = np.zeros(0, dtype=bool)
        self._iterations = 0
        self._kept = 0
        self._h = 0

    @staticmethod
    def _rows(a, name):
        """a 3 x N array (numpy or a device tensor) as N x 3 fp64 rows on the device"""
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise RuntimeError(f"{name}: expected a tensor on the ROCm device (no CPU path exists)")
            t = a.to(torch.float64)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        if t.dim() != 2 or t.shape[0] != 3:
            raise ValueError(f"{name}: expected a 3 x N array")
        return t.t().contiguous()

    def solve(self, src, dst) -> RegistrationSolution:
        """src, dst: 3 x N (column i is correspondence i).  Returns the solution ``getSolution()`` returns afterwards."""
        return self.solve_rows(self._rows(src, "src"), self._rows(dst, "dst"))

    def solve_rows(self, s: torch.Tensor, d: torch.Tensor) -> RegistrationSolution:
        """``solve`` on N x 3 fp64 rows that are on the device already (what the registration methods hold)."""
        self.reset()
        p = self.params
        n = s.shape[0]
        if d.shape[0] != n:
            raise ValueError("src and dst must have the same number of columns")
        if n > ops.TEASER_MAX_N:
            raise ValueError(f"{n} correspondences: at most {ops.TEASER_MAX_N} (the bit matrix of the consistency graph)")
        if n <= 1:
            return self._solution                                         # no measurement: invalid, as TEASER++ aborts
        adj, deg = ops.teaser_graph(s, d, p.noise_bound, p.cbar2)
        kept, info = ops.teaser_reduce(adj, deg)
        h, k = (int(x) for x in info.cpu().numpy())                       # read-back 1
        self._h, self._kept = h, k
        if h <= 1:                                                        # no edge at all: the clique is a single vertex
            self._clique = np.zeros(1, dtype=np.int32)
            return self._solution
        kept = kept[:k].contiguous()
        sub = ops.teaser_submatrix(adj, kept)
        packed = torch.cat((kept.to(torch.int64), sub.reshape(-1))).cpu().numpy()   # read-back 2
        clique = ops.teaser_max_clique_host(packed[k:], packed[:k].astype(np.int32), known=h, node_limit=self.node_limit)
        self._clique = clique
        if len(clique) <= 1:
            return self._solution
        R, w, it, v = ops.teaser_gnc(s, d, torch.from_numpy(clique).to(s.device), p.noise_bound, p.rotation_gnc_factor,
                                     p.rotation_max_iterations, p.rotation_cost_threshold)
        m = len(clique) - 1
        out = torch.cat((R.reshape(-1), w, v.reshape(-1), it.to(torch.float64))).cpu().numpy()   # read-back 3
        self._weights = out[9:9 + m].copy()
        self._iterations = int(out[-1])
        if self._iterations < 0:
            raise RuntimeError("teaser_gnc: a clique index outside the correspondences")
        t, t_in = ops.teaser_tls_translation_host(out[9 + m:9 + m + 3 * (m + 1)].reshape(-1, 3), p.noise_bound * math.sqrt(p.cbar2))
        self._translation_inliers = t_in
        sol = self._solution
        sol.rotation = out[:9].reshape(3, 3).copy()
        sol.translation = t
        sol.valid = True
        return sol

    def getSolution(self) -> RegistrationSolution:
        return self._solution

    def getInlierMaxClique(self):
        """the correspondences of the maximum clique, ascending (a list of ints, as the library returns)"""
        return [int(i) for i in self._clique]

    def getRotationInliersMask(self) -> np.ndarray:
        """over the chain measurements of the clique (one fewer than its members): GNC weight >= 0.5"""
        return self._weights >= 0.5

    def getTranslationInliersMask(self) -> np.ndarray:
        """over the members of the clique"""
        return self._translation_inliers.copy()

    def getRotationIterations(self) -> int:
        return self._iterations
