"""Mirror of kiss_icp.mapping (src/kiss-icp/python/kiss_icp/mapping.py:30-131) for the calls the
registration path makes: ``get_voxel_hash_map``, ``VoxelHashMap.add_points``, ``.point_cloud``,
``.point_cloud_n`` and ``.get_vfm_correspondences`` (C++: VoxelHashMap.cpp:461-626, 628-676,
733-770; binding kiss_icp_pybind.cpp:75-129).

The map keeps at most ``max_points_per_voxel`` points per voxel in insertion order
(VoxelHashMap.hpp:55-62).  ``point_cloud*()`` and the row numbering of the descriptor search follow
the reference's container: voxels in ``tsl::robin_map`` iteration order (a default-constructed map
that grew by doubling, VoxelHash of VoxelHashMap.hpp:72-77), the points of a voxel in insertion
order (csrc/voxel.hip ``vfm_voxel_robin``).  The map state is a pure function of the sequence of
kept points, so it is recomputed from that sequence when points were added.  The descriptor search
runs on the GPU through the C ABI; besides the reference's (source, target) coordinate pair the
indices are available (``get_vfm_correspondence_indices``), which makes the KD-tree index recovery
of registration_node.py:288-317 unnecessary.

``update`` and ``remove_far_away_points`` (mapping.py:59-75, 89-90) turn a map into the odometry's local map: from then on it lives as
the sorted-key grid ICP searches, updated in place on the device (csrc/odometry.hip ``vfm_icp_grid_update``).  The 387-column map keeps
its descriptor rows next to that grid, in the grid's order, and every update moves them along with the points
(``vfm_icp_grid_update_src`` + ``vfm_rows_merge``).

``descriptor_mode="weighted"`` (default ``"seeded"``: everything above) makes the wide rows the reference's ``map_x_``
(VoxelHashMap.cpp:717-731, 759-770, 789-795): rows of any width 3 + D, D >= 1, are kept as such a local map -- the same grid, the same two
enqueues -- and searched by the descriptor-weighted RegisterFrame (``icp.register_frame`` on the map, csrc/icp_rows.hip), for which the map
keeps every row's norm and "element sum != 0" flag, computed on the device (``weighted_operand``).  ``empty_x()`` tells whether it holds rows.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from .voxelization import to_device_rows


DESCRIPTOR_MODES = ("seeded", "weighted")


def check_descriptor_mode(mode) -> str:
    if mode not in DESCRIPTOR_MODES:
        raise ValueError(f"descriptor_mode: expected one of {DESCRIPTOR_MODES}, got {mode!r}")
    return mode


def get_voxel_hash_map(config, descriptor_mode="seeded"):
    return VoxelHashMap(voxel_size=config.mapping.voxel_size, max_distance=config.data.max_range,
                        max_points_per_voxel=config.mapping.max_points_per_voxel, descriptor_mode=descriptor_mode)


class VoxelHashMap:
    quiet = False  # the reference prints a stats line per search (VoxelHashMap.cpp:613-616)
    HALF_LIMIT = 24.0  # surviving chunks per query up to which a map's searches take the half-width coarse pass (pipeline.py's rule)

    def __init__(self, voxel_size: float, max_distance: float, max_points_per_voxel: int, descriptor_mode: str = "seeded"):
        # "seeded": wide rows are the reference's map_n_ (387 columns as a local map, the descriptor-seeded RegisterFrame); "weighted": they
        # are its map_x_ -- rows of any width 3 + D, D >= 1, as a local map, searched by the descriptor-weighted RegisterFrame
        self.descriptor_mode = check_descriptor_mode(descriptor_mode)
        self.voxel_size = float(voxel_size)
        self.max_distance = float(max_distance)
        self.max_points_per_voxel = int(max_points_per_voxel)
        self.clear()

    # ------------------------------------------------------------------ container
    def clear(self):
        # kind -> list of (rows, xyz64) device tensors in insertion order (3-D and N-D points live in separate maps);
        # the rows keep the dtype they were given in (see voxelization.to_device_rows)
        self._chunks = {}
        self._ordered = {}      # kind -> (rows, xyz64) in container iteration order (cache)
        self._dev = None        # cached (descriptors fp32, xyz fp64) of the N-D map (IndexFlatIP.add)
        self._prep = None       # ... and its prepared search operand (1 / |row| + the coarse pass's images), made at the first gated search
        self._half = None       # whether searches of this map take the half-width coarse pass (probed at the first search)
        self._load = None       # pinned int32[1]: load figure of the last gated search
        self._load_pending = None
        self._xyz = None        # cached xyz_map() (it carries the ICP grid register_frame builds from it)
        self._wide_grid = None  # the sorted-key grid of the N-D map once ``update`` ran on it: _chunks["n"] is then [(descriptors [n, d], grid.pts)]
        self._drop_icp_grids()

    def _drop_icp_grids(self):
        # the ICP grids register_frame keeps with the map (icp._grid_of, icp._register_frame_xd) are keyed on the kept-row count only:
        # a map refilled with as many other rows would be searched through the old coordinates and descriptors.  The weighted search's
        # norms and flags (weighted_operand) go with them, and are tied to the tensor of rows they were computed from besides
        self.__dict__.pop("_icp_grid", None)
        self.__dict__.pop("_icp_desc_grid", None)
        self.__dict__.pop("_wide_stats", None)

    @staticmethod
    def _kind(width: int) -> str:
        # mapping.py:77-85 routes 3 columns to map_, _point_size() (= 3 + DESCRIPTOR_SIZE, a compile-time 384 in
        # DescriptorSize.hpp:7) to map_n_ and other widths to map_x_.  Here the descriptor width is a run-time
        # property (configs C3 and C5 use 384 and 768): the first wide insert fixes it, a different width later is
        # an error, and map_x_ (never read by the path) does not exist.
        return "3" if width == 3 else "n"

    def empty(self):
        return not self._chunks.get("3")

    def empty_n(self):
        return not self._chunks.get("n")

    def empty_x(self):
        """VoxelHashMap::Empty_x: whether map_x_ -- the wide rows of a "weighted" map -- holds nothing (a "seeded" map has no map_x_)"""
        return self.descriptor_mode != "weighted" or self.empty_n()

    def add_points(self, points: np.ndarray):
        points = np.asarray(points)
        if points.ndim != 2 or points.shape[1] < 3:
            raise ValueError("Invalid shape")  # mapping.py:86
        if len(points) == 0:
            return
        kind = self._kind(points.shape[1])
        if kind == "n" and self.width_n() not in (None, points.shape[1]):
            raise ValueError("Invalid shape")      # (before anything is uploaded)
        if (kind == "n" and not self._chunks.get(kind) and len(points) >= self.OVERLAP_UPLOAD_FROM and points.dtype in (np.float32, np.float64)
                and torch.cuda.is_available()):
            return self._add_first_block_overlapped(points)
        self.add_points_device(*to_device_rows(points))

    # The FIRST block of a descriptor map (registration_node.py:402-403 builds the map from the whole local_map array in one call): the
    # container -- which points survive the per-voxel cap, and in which order the robin-map walks them -- is a function of the COORDINATES
    # alone (2.4 MB at 200 000 points), the upload is the 387-column rows (310 MB fp32: 5.5 ms of PCIe at 56 GB/s).  Round 6 (VERDICT r5
    # item 5, the cold call): the coordinates go first, the rows follow on a side stream from a helper thread (the copy call releases the
    # GIL), and the voxel cap + the growing map's replay (3.7 ms of dependent launches and read-backs, tools/time_api_cold.py) run under
    # the upload instead of behind it.  Same tensors as add_points_device + _cloud leave behind (tests/test_gpu_voxel.py, test_gpu_api.py).
    OVERLAP_UPLOAD_FROM = 50000
    _upload_pool = None
    _upload_streams = {}

    def _add_first_block_overlapped(self, points: np.ndarray):
        from concurrent.futures import ThreadPoolExecutor
        if VoxelHashMap._upload_pool is None:
            VoxelHashMap._upload_pool = ThreadPoolExecutor(1)
        pts = np.ascontiguousarray(points)
        main = torch.cuda.current_stream()
        dev = torch.cuda.current_device()
        # (one side stream per device for the life of the process: the caching allocator keeps a freed block for the stream it was allocated
        # on -- with a fresh stream per call every call paid a 310 MB hipMalloc)
        side = VoxelHashMap._upload_streams.get(dev)
        if side is None:
            side = VoxelHashMap._upload_streams[dev] = torch.cuda.Stream()

        def upload():
            with torch.cuda.device(dev), torch.cuda.stream(side):
                r = torch.from_numpy(pts).cuda()
                side.synchronize()
                return r
        fut = VoxelHashMap._upload_pool.submit(upload)
        try:
            xyz64 = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float64)).cuda()
            keep = ops.voxel_first(xyz64, self.voxel_size, self.max_points_per_voxel)
            xyz_kept = xyz64 if len(keep) == len(xyz64) else xyz64[keep]
            order = ops.voxel_robin(xyz_kept, self.voxel_size, self.max_points_per_voxel, reserve=False, hash_mul=ops.HASH_MAP)
        finally:
            rows = fut.result()
        main.wait_stream(side)
        rows.record_stream(main)
        rows_kept = rows if len(keep) == len(rows) else rows[keep]
        assert len(order) == len(rows_kept)
        self._chunks["n"] = [(rows_kept, xyz_kept)]
        self._ordered["n"] = (rows_kept[order], xyz_kept[order])
        self._dev = None
        self._prep = None
        self._xyz = None
        self._drop_icp_grids()

    def width_n(self) -> Optional[int]:
        """columns of the N-D map's rows (None: it is empty)"""
        if self.empty_n():
            return None
        rows = self._chunks["n"][0][0]
        return rows.shape[1] + (3 if self._wide_grid is not None else 0)

    def add_points_device(self, rows: torch.Tensor, xyz64: torch.Tensor):
        """add_points on rows that are already on the device (rows [n, w] fp32 / fp64, xyz64 [n, 3] fp64)."""
        kind = self._kind(rows.shape[1])
        if kind == "n" and self._wide_grid is not None and not self.empty_n():
            # an updated N-D map stays a grid: plain AddPoints through the update (no pose, nothing removed)
            if rows.shape[1] != self.width_n():
                raise ValueError("Invalid shape")
            return self._grid_update_n(rows[:, 3:].contiguous(), xyz64, None, None)
        # VoxelBlock::AddPoint keeps a point iff its voxel holds fewer than max_points_per_voxel points
        # (VoxelHashMap.hpp:55-62).  The points already stored come first and are all within the cap,
        # so "first K per voxel of [stored..., new...]" restricted to the new rows is exactly that rule.
        stored = self._chunks.get(kind, [])
        if stored and stored[0][0].shape[1] != rows.shape[1]:
            raise ValueError("Invalid shape")
        n_old = sum(len(r) for r, _ in stored)
        cat = torch.cat([x for _, x in stored] + [xyz64], dim=0) if n_old else xyz64
        keep = ops.voxel_first(cat, self.voxel_size, self.max_points_per_voxel)
        keep_new = keep[keep >= n_old] - n_old
        if stored and stored[0][0].dtype != rows.dtype:   # mixed precisions: everything to double, as pybind would
            stored[:] = [(r.double(), x) for r, x in stored]
            rows = rows.double()
        self._chunks.setdefault(kind, []).append((rows[keep_new], xyz64[keep_new]))
        self._ordered.pop(kind, None)
        self._dev = None
        self._prep = None
        self._xyz = None
        self._drop_icp_grids()

    # ------------------------------------------------------------------ the local map of the odometry
    # VoxelHashMap::Update (VoxelHashMap.cpp:693-699: AddPoints of the posed points, then RemovePointsFarFromLocation of the pose's
    # translation) for the 3-D map.  Both calls run through vfm_icp_grid_update on the sorted-key grid that ICP searches; from the first
    # of them on the map KEEPS that grid on the device (icp._grid_of finds it and does not rebuild), and its stored points are the
    # grid's, in (voxel key, insertion) order -- which is what point_cloud() then returns: the reference's set of points, not its
    # robin-map order after erasures.  Every far voxel goes, where the reference's erase-while-iterating keeps some until
    # the next call.  A map on which neither was called is untouched by any of this.
    #
    # The 387-column map (VoxelHashMap.cpp:701-715, 746-757, 781-787) follows the same rule with its descriptor rows as a payload: the grid
    # (keys, start, fp64 points) is kept in ``_wide_grid``, the descriptor columns alone as one contiguous [n, 384] tensor in the rows' dtype
    # and the grid's order -- (voxel key, insertion), the row numbering of the searches from then on (ties to the lower row).  The update
    # says where every output point came from and vfm_rows_merge moves the rows: two enqueues, one 6-int read-back.  A map filled by
    # add_points converts at its first update (its kept rows enter an empty grid in insertion order).  Other widths (the reference's map_x_)
    # are kept as a local map by a map made with descriptor_mode="weighted" only: there every width 3 + D, D >= 1, takes this path.
    def update(self, points, pose: np.ndarray = np.eye(4)):
        """mapping.py:59-75 for 3-column points (numpy, or fp64 [n, 3] on the device) and for rows of icp.POINT_SIZE = 387 columns (numpy
        or a device tensor, float32 or float64); a map made with descriptor_mode="weighted" takes rows of any width 3 + D, D >= 1, instead
        -- the first wide rows fix the width, another one later is ValueError("Invalid shape")"""
        from .icp import POINT_SIZE
        if not isinstance(points, torch.Tensor):
            points = np.asarray(points)
        if points.ndim != 2 or points.shape[1] < 3:
            raise ValueError("Invalid shape")  # mapping.py:73
        weighted = self.descriptor_mode == "weighted"
        if weighted and points.shape[1] > 3:
            have = self.width_n()
            if have is not None and have != points.shape[1]:      # (before anything is uploaded)
                raise ValueError("Invalid shape")
        elif points.shape[1] not in (3, POINT_SIZE):
            raise NotImplementedError(f"update of a local map that carries descriptors: rows of width {points.shape[1]} (only 3-column "
                                      f"points and {POINT_SIZE}-column rows are kept in a device-resident local map)")
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        if pose.shape != (4, 4):
            raise ValueError("expected a 4 x 4 pose")
        if points.shape[1] == POINT_SIZE or (weighted and points.shape[1] > 3):
            if isinstance(points, torch.Tensor):
                if not points.is_cuda:
                    raise RuntimeError("points: expected a tensor on the ROCm device (no CPU path exists)")
                rows = points if points.dtype in (torch.float32, torch.float64) else points.double()
                xyz = rows[:, :3].double().contiguous()
            else:
                rows, xyz = to_device_rows(points)
            return self._grid_update_n(rows[:, 3:].contiguous(), xyz, pose, pose[:3, 3])
        xyz = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).cuda()
        return self._grid_update(xyz.contiguous(), pose, pose[:3, 3])

    def remove_far_away_points(self, origin):
        """mapping.py:89-90: drop every voxel whose first point is farther than max_distance from ``origin`` -- of the 3-D map and of the
        387-column one (VoxelHashMap.cpp:772-787)"""
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        if origin.shape != (3,):
            raise ValueError("expected an origin of 3 values")
        if self.empty_n() or not self._is_local_width(self.width_n() - 3):      # (rows of another width are no local map: left alone)
            return self._grid_update(None, None, origin)
        first = None
        if not self.empty():
            self._grid_update(None, None, origin)
            first = self.last_update
        self._grid_update_n(None, None, None, origin)
        if first is not None:
            self.last_update = {k: v + first[k] for k, v in self.last_update.items()}

    @staticmethod
    def _descriptor_width() -> int:
        from .icp import POINT_SIZE
        return POINT_SIZE - 3

    def _is_local_width(self, d: int) -> bool:
        """whether rows of ``d`` descriptor columns are kept as a device-resident local map"""
        return d >= 1 if self.descriptor_mode == "weighted" else d == self._descriptor_width()

    def _read_update_info(self, info):
        from .icp import OUT_OF_RANGE_MESSAGE
        info_h = getattr(ops._tls, "icp_update_info", None)   # page-locked: the update's one read-back
        if info_h is None:
            info_h = ops._tls.icp_update_info = torch.zeros(6, dtype=torch.int32).pin_memory()
        info_h.copy_(info, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        vals = info_h.tolist()
        if vals[2]:
            raise ValueError(OUT_OF_RANGE_MESSAGE)   # (the map is left as it was)
        return vals

    def _install_wide(self, out):
        """the N-D map := the grid and payload rows an update returned (its one read-back happens here)"""
        from .icp import VoxelGridDevice
        n_voxels, n_kept, _, added, voxels_removed, points_removed = self._read_update_info(out["info"])
        grid = VoxelGridDevice.__new__(VoxelGridDevice)
        grid.voxel_size = self.voxel_size
        grid.n_voxels, grid.n_kept = n_voxels, n_kept
        grid.keys, grid.start, grid.pts = out["keys"][:n_voxels], out["start"][:n_voxels + 1], out["pts"][:n_kept]
        desc = out["rows"][:n_kept]
        self._wide_grid = grid if n_kept else None
        self._chunks["n"] = [(desc, grid.pts)] if n_kept else []
        if n_kept:
            self._ordered["n"] = (desc, grid.pts)
        else:
            self._ordered.pop("n", None)
        self._dev = None        # the search operand is prepared again for the whole map at the next search
        self._prep = None
        self._half = None
        self._xyz = None
        self.__dict__.pop("_icp_desc_grid", None)
        self.__dict__.pop("_wide_stats", None)     # (the weighted search's norms and flags: of the rows that were here before)
        self.last_update = dict(points_added=added, voxels_removed=voxels_removed, points_removed=points_removed)

    def _grid_update_n(self, desc, xyz, pose, origin):
        """Update / AddPoints / RemovePointsFarFromLocation of the N-D map: ``desc`` [m, d] contiguous and ``xyz`` fp64 [m, 3] on the device
        (None: no new points), ``pose`` a host 4 x 4 or None, ``origin`` 3 host values or None (nothing is removed)"""
        if desc is not None and desc.shape[0] == 0:
            desc = xyz = None
        self._ensure_wide_grid()
        g = self._wide_grid
        if g is None and desc is None:
            self.last_update = dict(points_added=0, voxels_removed=0, points_removed=0)
            return
        old = None if g is None else self._chunks["n"][0][0]
        if old is not None and desc is not None:
            if old.shape[1] != desc.shape[1]:
                raise ValueError("Invalid shape")
            if old.dtype != desc.dtype:      # mixed precisions: everything to double, as add_points_device does
                old, desc = old.double(), desc.double()
        out = ops.icp_grid_update(None if g is None else g.keys, None if g is None else g.start, None if g is None else g.pts, xyz, pose,
                                  self.voxel_size, self.max_points_per_voxel, origin, self.max_distance, rows_old=old, rows_new=desc)
        self._install_wide(out)

    def _ensure_wide_grid(self):
        """a wide map that add_points filled becomes the grid + descriptor columns an updated map is (nothing happens to one that is, or
        to an empty one)"""
        if self._wide_grid is None and not self.empty_n():
            # the first update of a map add_points filled: every stored row is a kept one, so they all enter an empty grid, in insertion order
            chunks = self._chunks["n"]
            rows = torch.cat([r for r, _ in chunks], dim=0) if len(chunks) > 1 else chunks[0][0]
            old_xyz = torch.cat([x for _, x in chunks], dim=0) if len(chunks) > 1 else chunks[0][1]
            if not self._is_local_width(rows.shape[1] - 3):
                raise NotImplementedError(f"update of a local map that carries descriptors: rows of width {rows.shape[1]}")
            self._install_wide(ops.icp_grid_update(None, None, None, old_xyz.contiguous(), None, self.voxel_size, self.max_points_per_voxel, None,
                                                   self.max_distance, rows_new=rows[:, 3:].contiguous()))

    def weighted_operand(self):
        """What the descriptor-weighted search reads of a "weighted" map, all on the device: (grid, descriptor rows [n_kept, D] in the
        grid's order and the rows' dtype, norm fp64[n_kept], "element sum != 0" uint8[n_kept]).  The statistics are computed on the device
        for the whole map (``vfm_icp_rows_stats``) at the first search after the map changed and kept until it changes again: they belong
        to the very tensor of rows they were computed from (profiles/odometry_weighted_timing.md has the figures behind "recomputed, not
        carried through the update").  A map that add_points filled becomes a grid here, as at its first update."""
        if self.descriptor_mode != "weighted":
            raise RuntimeError("weighted_operand: the map was not made with descriptor_mode=\"weighted\"")
        self._ensure_wide_grid()
        if self._wide_grid is None:
            return None
        desc = self._chunks["n"][0][0]
        stats = self.__dict__.get("_wide_stats")
        if stats is None or stats[0] is not desc:
            stats = self._wide_stats = (desc,) + ops.icp_rows_stats(desc)
        return self._wide_grid, desc, stats[1], stats[2]

    def _grid_update(self, xyz, pose, origin):
        from .icp import VoxelGridDevice, _grid_of
        g = _grid_of(self) if not self.empty() else None
        if xyz is not None and xyz.shape[0] == 0:
            xyz = None
        out = ops.icp_grid_update(None if g is None else g.keys, None if g is None else g.start, None if g is None else g.pts, xyz, pose,
                                  self.voxel_size, self.max_points_per_voxel, origin, self.max_distance)
        n_voxels, n_kept, _, added, voxels_removed, points_removed = self._read_update_info(out["info"])
        grid = VoxelGridDevice.__new__(VoxelGridDevice)
        grid.voxel_size = self.voxel_size
        grid.n_voxels, grid.n_kept = n_voxels, n_kept
        grid.keys, grid.start, grid.pts = out["keys"][:n_voxels], out["start"][:n_voxels + 1], out["pts"][:n_kept]
        self._chunks["3"] = [(grid.pts, grid.pts)] if n_kept else []
        if n_kept:
            self._ordered["3"] = (grid.pts, grid.pts)
        else:
            self._ordered.pop("3", None)
        self.__dict__.pop("_icp_grid", None)
        self._icp_grid = (n_kept, grid)
        self.last_update = dict(points_added=added, voxels_removed=voxels_removed, points_removed=points_removed)

    def _cloud(self, kind: str):
        """(rows, xyz64) of one of the maps as the reference walks it (VoxelHashMap.cpp:628-676), on the device."""
        chunks = self._chunks.get(kind)
        if not chunks:
            return None
        if kind not in self._ordered:
            rows = torch.cat([r for r, _ in chunks], dim=0) if len(chunks) > 1 else chunks[0][0]
            xyz = torch.cat([x for _, x in chunks], dim=0) if len(chunks) > 1 else chunks[0][1]
            # every stored row is a kept one: replaying them reproduces the container (voxels are created
            # by their first point, which is always kept)
            order = ops.voxel_robin(xyz, self.voxel_size, self.max_points_per_voxel, reserve=False, hash_mul=ops.HASH_MAP)
            assert len(order) == len(rows)
            self._ordered[kind] = (rows[order], xyz[order])
        return self._ordered[kind]

    def xyz_map(self) -> "VoxelHashMap":
        """The 3-D map ``add_points(points[:, :3])`` would build from the same rows (registration_node.py:290-293 builds
        it next to the N-D one): same voxels, same kept points, same container order -- shared, not recomputed."""
        if self._xyz is not None:   # (kept: a scene's map serves many scans, and the ICP grid built from it stays with it)
            return self._xyz
        m = VoxelHashMap(self.voxel_size, self.max_distance, self.max_points_per_voxel)
        if self._wide_grid is not None and not self.empty_n():
            m._icp_grid = (self._wide_grid.n_kept, self._wide_grid)     # the updated grid itself: icp._grid_of does not rebuild it
        m._chunks["3"] = [(x, x) for _, x in self._chunks.get("n", [])]
        if "n" in self._ordered:
            m._ordered["3"] = (self._ordered["n"][1], self._ordered["n"][1])
        self._xyz = m
        return m

    def point_cloud_device(self) -> Optional[torch.Tensor]:
        for kind in ("3", "n"):  # VoxelHashMap.cpp:631-659: map_, else map_n_ (else map_x_)
            c = self._cloud(kind)
            if c is not None:
                return c[1]
        return None

    def point_cloud(self) -> np.ndarray:
        x = self.point_cloud_device()
        return x.cpu().numpy() if x is not None else np.zeros((0, 3))

    def point_cloud_n(self) -> np.ndarray:
        c = self._cloud("n")  # VoxelHashMap.cpp:664-676
        if c is None:
            return np.zeros((0, 3))
        if self._wide_grid is not None:
            return torch.cat((c[1], c[0].double()), dim=1).cpu().numpy()
        out = c[0].double().cpu().numpy()
        out[:, :3] = c[1].cpu().numpy()
        return out

    # ------------------------------------------------------------------ search
    def _device_map(self):
        if self._dev is None:
            rows, xyz = self._cloud("n")
            if self._wide_grid is not None:       # the descriptor columns alone, contiguous: float32 rows go to the search as they are
                self._dev = (rows if rows.dtype == torch.float32 else rows.float(), xyz)
            else:
                self._dev = (rows[:, 3:].float().contiguous(), xyz)   # VoxelHashMap.cpp:472-473: static_cast<float>
        return self._dev

    def search_device(self, q_rows: Optional[torch.Tensor], min_cosine_similarity: float, resolve_all: bool = False,
                      q_desc: Optional[torch.Tensor] = None):
        """Device form of the search: (query_idx int64[K], map_idx int64[K], sim fp32[N]) as device tensors.  ``sim`` is the
        best cosine of every query that can reach ``min_cosine_similarity`` and the sentinel -2.0 for queries that provably
        cannot (the gated search does not resolve them; the correspondences are unaffected).  ``resolve_all=True`` runs the
        ungated search instead: ``sim`` is then the reference's D array (VoxelHashMap.cpp:486-495) for every query."""
        b_desc, _ = self._device_map()
        if q_desc is not None:     # the descriptor columns alone, already float32 (a caller that keeps the coordinates elsewhere)
            if q_desc.dim() != 2 or q_desc.shape[1] != b_desc.shape[1] or q_desc.dtype != torch.float32:
                raise RuntimeError("Unable to cast Python instance to C++ type: expected %d float32 descriptor columns" % b_desc.shape[1])
            q_desc = q_desc.contiguous()
        else:
            if q_rows.dim() != 2 or q_rows.shape[1] != b_desc.shape[1] + 3:
                raise RuntimeError("Unable to cast Python instance to C++ type: expected %d columns"
                                   % (b_desc.shape[1] + 3))  # py::cast_error, stl_vector_eigen.h:76-78
            q_desc = q_rows[:, 3:].float().contiguous()            # VoxelHashMap.cpp:478-481
        d = q_desc.shape[1]
        prec = ops.FAST if (d % 128 == 0 and 128 <= d <= 768) else ops.EXACT
        # only matches with cosine >= min_cosine_similarity leave this function (VoxelHashMap.cpp:501-511): the gated search
        # leaves queries that provably cannot reach it unresolved (sim = -2.0 in the returned array)
        gate = float(np.nextafter(np.float32(min_cosine_similarity), np.float32(-np.inf)))
        if prec == ops.FAST and not resolve_all and ops.gated_split_ok(d) and q_desc.shape[0] > 0:
            # the map is searched by every scan of a scene (RN:587-589): its operand is prepared once (IndexFlatIP.add happens once in the
            # reference too, VoxelHashMap.cpp:486-487), a call prepares its few hundred query rows and runs the gated search on both
            if self._prep is None or self._prep.x is not b_desc:
                self._prep = ops.PreparedRows(b_desc)
                self._half = None   # not yet probed for this map
            qp = ops.PreparedRows(q_desc)
            if self._load is None:
                self._load = torch.zeros(1, dtype=torch.int32).pin_memory()
            n = q_desc.shape[0]
            if self._half is None:
                # Half-width coarse pass (VFM_RECORDS_HALF: the int8 image of the first d / 2 columns, the other half bounded by
                # Cauchy-Schwarz against the gate) where it prunes: half the coarse kernel, which is most of a search of ~10^3 queries.
                # On descriptors that are alike every chunk survives its bound and the pass is far slower than the full-width one,
                # so the first search of a map PROBES it (its coarse pass + a count of the survivors, one read-back) -- the rule
                # of vfmreg/pipeline.py's `auto`: at most HALF_LIMIT surviving chunks per query.
                ops.match_probe_half(qp, self._prep, gate, self._load)
                torch.cuda.current_stream().synchronize()
                self._half = int(self._load.item()) <= self.HALF_LIMIT * n
            records = 3 if self._half else 0    # VFM_RECORDS_HALF / VFM_RECORDS_BEST
            idx, sim = ops.match_search_gated(qp, self._prep, gate, records=records, rescans_out=self._load)
            self._load_pending = (records, n)
        else:
            idx, sim = ops.match_ip_top1(q_desc, b_desc, prec, gate=gate if (prec == ops.FAST and not resolve_all) else None)
        r = ops.threshold_compact(sim, idx, float(min_cosine_similarity), want_corres=True)
        k = int(r["count"].item())
        if self._load_pending is not None:      # (the read-back above has passed the search: its load figure is in)
            records, n = self._load_pending
            self._load_pending = None
            if records == 3 and int(self._load.item()) > self.HALF_LIMIT * n:
                self._half = False              # this scan's descriptors do not prune at half width: full width from the next search on
        corres = r["corres"][:k]
        return corres[:, 0].long(), corres[:, 1].long(), sim

    def search_device_topk(self, q_rows: Optional[torch.Tensor], min_cosine_similarity: float, k: int,
                           q_desc: Optional[torch.Tensor] = None):
        """The search with k candidates per point, as VoxelHashMap.cpp:491-511, 587-600 is written (``I[i * k + j]``; the reference sets
        k = 1): (query_idx int64[K], map_idx int64[K], rank int64[K], sim fp32[N, k]) as device tensors.  ``sim`` is faiss' D array --
        every query's k best cosines, descending, equal ones to the lower map row, (-1, lowest float32) behind the last map row --;
        an entry is a correspondence iff ``!(sim < min_cosine_similarity)`` (VoxelHashMap.cpp:503), and the pairs come query-major,
        rank-minor (VoxelHashMap.cpp:590-600).  No query is left unresolved: the gate is applied to the result."""
        b_desc, _ = self._device_map()
        if q_desc is not None:
            if q_desc.dim() != 2 or q_desc.shape[1] != b_desc.shape[1] or q_desc.dtype != torch.float32:
                raise RuntimeError("Unable to cast Python instance to C++ type: expected %d float32 descriptor columns" % b_desc.shape[1])
            q_desc = q_desc.contiguous()
        else:
            if q_rows.dim() != 2 or q_rows.shape[1] != b_desc.shape[1] + 3:
                raise RuntimeError("Unable to cast Python instance to C++ type: expected %d columns" % (b_desc.shape[1] + 3))
            q_desc = q_rows[:, 3:].float().contiguous()            # VoxelHashMap.cpp:478-481
        if q_desc.shape[1] in ops.MATCH_TOPK_FAST_WIDTHS and q_desc.shape[0] > 0 and b_desc.shape[0] > 0:
            # the map's operand is prepared once and kept, under search_device's rule -- the top-1 and the k-best search of a map share
            # one image --; a call prepares its query rows alone
            if self._prep is None or self._prep.x is not b_desc:
                self._prep = ops.PreparedRows(b_desc)
                self._half = None   # not yet probed for this map
            idx, sim = ops.match_ip_topk_prepared(ops.PreparedRows(q_desc), self._prep, k)
        else:
            prec = ops.FAST if q_desc.shape[1] in ops.MATCH_TOPK_FAST_WIDTHS else ops.EXACT
            idx, sim = ops.match_ip_topk(q_desc, b_desc, k, prec)
        valid = ~(sim.double() < float(min_cosine_similarity)) & (idx >= 0)   # (the padding never passes a gate a cosine can reach)
        at = torch.nonzero(valid)                                  # row-major: query-major, rank-minor
        return at[:, 0], idx[valid], at[:, 1], sim

    def get_vfm_correspondence_indices_topk(self, points: np.ndarray, min_cosine_similarity: float, k: int):
        """(query_idx[K], map_idx[K], rank[K], sim[N, k]) -- ``get_vfm_correspondence_indices`` with k candidates per point, in the
        reference's emission order (see ``search_device_topk``)."""
        points = np.asarray(points)
        if self._cloud("n") is None or points.ndim != 2:
            raise RuntimeError("Unable to cast Python instance to C++ type")
        qi, mi, rank, sim = self.search_device_topk(to_device_rows(points)[0], min_cosine_similarity, k)
        return qi.cpu().numpy(), mi.cpu().numpy(), rank.cpu().numpy(), sim.cpu().numpy()

    def get_vfm_correspondence_indices(self, points: np.ndarray, min_cosine_similarity: float, resolve_all: bool = False):
        """(query_idx[K], map_idx[K], sim[N]) -- the indices behind get_vfm_correspondences.  ``sim[i]`` = -2.0 marks a query
        that provably has no match at the threshold (see ``search_device``); ``resolve_all=True`` returns every best cosine."""
        points = np.asarray(points)
        if self._cloud("n") is None or points.ndim != 2:
            raise RuntimeError("Unable to cast Python instance to C++ type")
        qi, mi, sim = self.search_device(to_device_rows(points)[0], min_cosine_similarity, resolve_all)
        return qi.cpu().numpy(), mi.cpu().numpy(), sim.cpu().numpy()

    def get_vfm_correspondences(self, points: np.ndarray, max_correspondance_distance: float
                                ) -> Tuple[np.ndarray, np.ndarray]:
        """Pair of {source, target} coordinates (mapping.py:120-131); the float is the cosine
        threshold despite its name (kiss_icp_pybind.cpp:128-129)."""
        points = np.asarray(points)
        # the stats line of VoxelHashMap.cpp:613-616 prints the mean of the best cosine over ALL queries (VoxelHashMap.cpp:588-602),
        # so the printing form resolves every query; ``quiet`` callers take the gated search (same correspondences)
        qi, mi, sim = self.get_vfm_correspondence_indices(points, max_correspondance_distance, resolve_all=not self.quiet)
        m_xyz = self._device_map()[1]
        if not self.quiet:
            print(f"Points: {len(points)} | Corrs.: {len(qi)} | Outliers: 0 | Mean sim.: {float(sim.mean()) if len(sim) else 0.0}")
        return (np.asarray(points[qi, :3], dtype=np.float64),
                m_xyz[torch.from_numpy(mi).to(m_xyz.device)].cpu().numpy())
