"""Step driver: the master / worker protocol of src/semiimplicit.jl:126-332 with one radial tile per GPU.

The reference runs one Julia worker per tile, a unidirectional RemoteChannel chain for the 3-coefficient halo
(src/semiimplicit.jl:203-219, 320-329), a SharedArray for the patch-level sum (:229, :272-282) and a redundant
patch solve on every worker (:285).  Here a tile is a libscythe_hip handle and the exchange is done on device
buffers: halo rows by point-to-point send/recv, owned rows by an in-place all-gather, both over
torch.distributed (backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in the CPU tests).
"""
import collections
import dataclasses
import os
import time

import numpy as np

from .model import (Distribution, Grid, GridParameters, ModelParameters, Statistics, calcTileSizes, checkCFL, comm_unique_id, getGridpoints,
                    program_of_outputs, thermo_programs)

Located = collections.namedtuple("Located", "pos value status")
WindRadii = collections.namedtuple("WindRadii", "thresholds azimuths radii quadrants")
VortexProfile = collections.namedtuple("VortexProfile", "centre radii radial tangential wave1 wave2 status")
Cfad = collections.namedtuple("Cfad", "frac under over nan area edges")
Exceedance = collections.namedtuple("Exceedance", "thresholds measure integral")
Quantile = collections.namedtuple("Quantile", "lo hi passes nan_count measure")
Swath = collections.namedtuple("Swath", "speed time samples")


class PatchLayout:
    """Which patch rows (radial nodes) each tile computes, owns and sends (calcPatchMap / calcHaloMap,
    src/semiimplicit.jl:79-86), and where they sit in the all-gather buffer."""

    def __init__(self, patch: GridParameters, num_tiles: int, n_cols: int = 0, split="reference"):
        """split = "reference": calcTileSizes (cells split evenly, or gridpoints balanced on native rings).
        split = "cost" (uniform ring tables only): cells whose rings still have a growing wavenumber truncation
        (ring index < L/2 - 1) run the ring-wise kernels, which cost about 1.6x the node-space path per ring, so the inner
        tiles get proportionally fewer cells - the same idea as the reference's gridpoint balancing (src/semiimplicit.jl:144)."""
        ts = calcTileSizes(patch, num_tiles)
        if split == "cost" and num_tiles > 1 and patch.ring_uniform_L > 0 and "L" in patch.geometry:
            ts = _cost_balanced_tiles(patch, num_tiles, ts)
        elif split not in ("reference", "cost"):
            raise ValueError("split must be 'reference' or 'cost'")
        self.num_tiles = num_tiles
        self.ncells = [int(ts[2, t]) for t in range(num_tiles)]
        self.cell0 = [int(ts[3, t]) - 1 for t in range(num_tiles)]
        self.tile_sizes = ts
        self.b_rDim = patch.num_cells + 3
        self.max_rows = max(self.ncells) + 3
        self.n_cols = n_cols

    def rows(self, t):
        return self.ncells[t] + 3

    def owned_rows(self, t):
        return self.ncells[t] + (3 if t == self.num_tiles - 1 else 0)

    def row_offsets(self, n_cols=None):
        """Element offset of patch row m inside the [num_tiles][max_rows][n_cols] gather buffer."""
        n_cols = n_cols or self.n_cols
        off = np.zeros(self.b_rDim, dtype=np.int64)
        for t in range(self.num_tiles):
            for j in range(self.owned_rows(t)):
                off[self.cell0[t] + j] = (t * self.max_rows + j) * n_cols
        return off


def _cost_balanced_tiles(patch, n, ts_ref, inner_weight=1.6):
    nc = patch.num_cells
    kcap = patch.ring_uniform_L // 2 - 1
    w = np.array([inner_weight if 3 * c < kcap else 1.0 for c in range(nc)])
    cum = np.concatenate([[0.0], np.cumsum(w)])
    bounds = [0]
    for t in range(1, n):
        c = int(np.searchsorted(cum, cum[-1] * t / n))
        c = max(c, bounds[-1] + 3)                    # at least 3 cells per tile (calcTileSizes' rule)
        c = min(c, nc - 3 * (n - t))
        bounds.append(c)
    bounds.append(nc)
    DX = (patch.xmax - patch.xmin) / nc
    pts_per_cell = 3 * patch.ring_uniform_L * max(patch.zDim, 1) if "Z" in patch.geometry else 3 * patch.ring_uniform_L
    ts = np.zeros_like(ts_ref)
    for t in range(n):
        c0, c1 = bounds[t], bounds[t + 1]
        ts[:, t] = (patch.xmin + c0 * DX, patch.xmin + c1 * DX, c1 - c0, c0 + 1, (c1 - c0) * pts_per_cell)
    return ts


def _torch():
    import torch
    return torch


class LocalExchange:
    """All tiles live in this process on one device (used by single-GPU tests of the tile protocol)."""

    def __init__(self, layout: PatchLayout, tiles, device):
        torch = _torch()
        self.layout, self.tiles = layout, tiles
        C = tiles[0].n_cols
        self.buf = torch.zeros((layout.num_tiles, layout.max_rows, C), dtype=torch.float64, device=device)
        ro = layout.row_offsets(C)
        for t, g in enumerate(tiles):
            g.bind_tile_b(self.buf[t].data_ptr())
            g.bind_patch_b(self.buf.data_ptr(), ro)

    def exchange(self):
        lay = self.layout
        for t in range(1, lay.num_tiles):
            n = lay.ncells[t - 1]
            self.tiles[t].halo_add(self.buf[t - 1, n:n + 3].data_ptr())


class DistExchange:
    """One tile per rank. Halo rows travel rank -> rank + 1, owned rows are all-gathered in place."""

    def __init__(self, layout: PatchLayout, tile: Grid, device, group=None):
        torch = _torch()
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        assert self.world == layout.num_tiles
        self.layout, self.tile = layout, tile
        C = tile.n_cols if tile is not None else layout.n_cols
        self.buf = torch.zeros((self.world, layout.max_rows, C), dtype=torch.float64, device=device)
        self.halo = torch.zeros((3, C), dtype=torch.float64, device=device)
        if tile is not None:
            tile.bind_tile_b(self.buf[self.rank].data_ptr())
            tile.bind_patch_b(self.buf.data_ptr(), layout.row_offsets(C))
        self.stage_host = (dist.get_backend(group) == "gloo" and self.buf.is_cuda)   # one-GPU rehearsal only

    def my_rows(self):
        return self.buf[self.rank]

    def exchange(self, halo_add=None):
        """halo_add(recv_tensor) adds the received rows into rows 0..2 of this tile (device kernel on the GPU path)."""
        dist, r, W = self.dist, self.rank, self.world
        if W > 1:
            ops = []
            n = self.layout.ncells[r]
            send = self.buf[r, n:n + 3]
            recv = self.halo
            if self.stage_host:
                send, recv = send.cpu(), self.halo.cpu()
            if r < W - 1:
                ops.append(dist.P2POp(dist.isend, send, r + 1, self.group))
            if r > 0:
                ops.append(dist.P2POp(dist.irecv, recv, r - 1, self.group))
            for w in dist.batch_isend_irecv(ops):
                w.wait()
            if r > 0:
                if self.stage_host:
                    self.halo.copy_(recv)
                if halo_add is not None:
                    halo_add(self.halo)
                else:
                    self.tile.halo_add(self.halo.data_ptr())
            if self.stage_host:
                full = self.buf.cpu()
                dist.all_gather_into_tensor(full.view(-1), full[r].reshape(-1).clone(), group=self.group)
                self.buf.copy_(full)
            else:
                dist.all_gather_into_tensor(self.buf.view(-1), self.buf[r].reshape(-1), group=self.group)


class A2ALayout:
    """Buffer geometry of the transposed solve for tile `me` (see include/scythe_hip.h, sx_a2a_*)."""

    def __init__(self, layout: PatchLayout, col_starts, me, rows=None):
        """rows = None: every tile moves all its ncells + 3 rows (transposed solve); rows = 10: the interface-only solve."""
        self.n = layout.num_tiles
        self.rows = [layout.rows(t) if rows is None else rows for t in range(self.n)]
        self.cw = [int(col_starts[d + 1] - col_starts[d]) for d in range(self.n)]
        self.me = me
        # tile side: [dest d][row][cw[d]];  owner side: [tile t][row][cw[me]]
        self.tile_split = [self.rows[me] * self.cw[d] for d in range(self.n)]
        self.owner_split = [self.rows[t] * self.cw[me] for t in range(self.n)]
        self.tile_elems = sum(self.tile_split)
        self.owner_elems = sum(self.owner_split)


IFACE_ROWS = 10     # rows per tile that travel in the interface-only solve (6 edge values + 4 foreign rows, sx_iface.hip)


def _kernels_of(tile, kind):
    """(first, middle, last) device stages around the two all-to-alls: pack / solve / unpack of the transposed solve or
    local solve / reduced system / correction of the interface-only solve."""
    if kind == "iface":
        return tile.iface_local, tile.iface_reduce, tile.iface_apply
    return tile.a2a_pack_b, tile.a2a_solve, tile.a2a_unpack_a


class LocalA2AExchange:
    """Transposed solve (kind "a2a") or interface-only solve (kind "iface") with all tiles in this process (single-GPU test
    of the kernels on either side of the two all-to-alls)."""

    def __init__(self, layout: PatchLayout, tiles, device, kind="a2a"):
        torch = _torch()
        self.tiles, self.kind = tiles, kind
        self.lay = []
        for t, g in enumerate(tiles):
            if kind == "iface":
                self.lay.append(A2ALayout(layout, g.iface_configure(layout.cell0, layout.ncells, t), t, rows=IFACE_ROWS))
            else:
                self.lay.append(A2ALayout(layout, g.a2a_configure(layout.cell0, layout.ncells, t), t))
        z = lambda n: torch.zeros(max(n, 1), dtype=torch.float64, device=device)
        self.tile_buf = [z(l.tile_elems) for l in self.lay]      # pack output / unpack input
        self.own_in = [z(l.owner_elems) for l in self.lay]
        self.own_out = [z(l.owner_elems) for l in self.lay]

    def _all_to_all(self, src, src_splits, dst, dst_splits):
        n = len(src)
        for s in range(n):
            so = 0
            for d in range(n):
                cnt = src_splits[s][d]
                do = sum(dst_splits[d][:s])
                dst[d][do:do + cnt] = src[s][so:so + cnt]
                so += cnt

    def exchange_and_solve(self):
        for g, b in zip(self.tiles, self.tile_buf):
            _kernels_of(g, self.kind)[0](b.data_ptr())
        self._all_to_all(self.tile_buf, [l.tile_split for l in self.lay], self.own_in, [l.owner_split for l in self.lay])
        for g, i, o in zip(self.tiles, self.own_in, self.own_out):
            _kernels_of(g, self.kind)[1](i.data_ptr(), o.data_ptr())
        self._all_to_all(self.own_out, [l.owner_split for l in self.lay], self.tile_buf, [l.tile_split for l in self.lay])
        for g, b in zip(self.tiles, self.tile_buf):
            _kernels_of(g, self.kind)[2](b.data_ptr())


class DistA2AExchange:
    """Transposed solve (kind "a2a") or interface-only solve (kind "iface"), one tile per rank: two all_to_all_single calls
    per step (RCCL over xGMI on the GPU box)."""

    def __init__(self, layout: PatchLayout, tile, device, group=None, col_starts=None, kind="a2a"):
        torch = _torch()
        import torch.distributed as dist
        self.dist, self.group, self.tile, self.kind = dist, group, tile, kind
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        assert self.world == layout.num_tiles
        if tile is not None:
            col_starts = (tile.iface_configure if kind == "iface" else tile.a2a_configure)(layout.cell0, layout.ncells, self.rank)
        self.lay = A2ALayout(layout, col_starts, self.rank, rows=IFACE_ROWS if kind == "iface" else None)
        z = lambda n: torch.zeros(max(n, 1), dtype=torch.float64, device=device)
        self.tile_buf, self.tile_buf2 = z(self.lay.tile_elems), z(self.lay.tile_elems)
        self.own_in, self.own_out = z(self.lay.owner_elems), z(self.lay.owner_elems)
        # gloo cannot move device tensors through all_to_all: stage through the host (rehearsal on one GPU only;
        # the production backend is "nccl" = RCCL, which takes the device buffers directly)
        self.stage_host = (dist.get_backend(group) == "gloo" and self.tile_buf.is_cuda)

    def _a2a(self, out, inp, out_split, in_split):
        out, inp = out[:sum(out_split)], inp[:sum(in_split)]        # a rank without columns keeps a 1-element placeholder buffer
        if self.stage_host:
            o = out.cpu()
            self.dist.all_to_all_single(o, inp.cpu(), out_split, in_split, group=self.group)
            out.copy_(o)
        else:
            self.dist.all_to_all_single(out, inp, out_split, in_split, group=self.group)

    def exchange_and_solve(self, pack=None, solve=None, unpack=None):
        """pack / solve / unpack default to the tile's device kernels; the CPU tests pass numpy stand-ins."""
        lay = self.lay
        k = _kernels_of(self.tile, self.kind) if self.tile is not None else (None, None, None)
        (pack or (lambda b: k[0](b.data_ptr())))(self.tile_buf)
        self._a2a(self.own_in, self.tile_buf, lay.owner_split, lay.tile_split)
        (solve or (lambda i, o: k[1](i.data_ptr(), o.data_ptr())))(self.own_in, self.own_out)
        self._a2a(self.tile_buf2, self.own_out, lay.tile_split, lay.owner_split)
        (unpack or (lambda b: k[2](b.data_ptr())))(self.tile_buf2)


class LibExchange:
    """One tile per rank, exchange done INSIDE libscythe_hip.so with RCCL on the tile's stream (sx_comm_init / sx_exchange):
    what a Julia host would use.  Only the 128-byte ncclUniqueId travels through the host-side launcher - here
    torch.distributed's store (any backend), in the reference's world the master's RemoteChannels."""

    def __init__(self, layout: PatchLayout, tile: Grid, mode, group=None, unique_id=None):
        self.tile, self.mode = tile, mode
        rank, world = 0, 1
        if unique_id is None:
            import torch.distributed as dist
            rank, world = dist.get_rank(group), dist.get_world_size(group)
            assert world == layout.num_tiles
            # Everything that can fail on one rank alone happens BEFORE the first collective, and the ranks agree on the outcome:
            # a rank that raised here while the others sat in the broadcast (or in ncclCommInitRank) would hang the job.
            err, uid = "", None
            try:
                tile.comm_prepare(layout.cell0, layout.ncells, rank, mode)      # librccl, tile table, buffers: not collective
                uid = comm_unique_id()                                          # ncclGetUniqueId: not collective either
            except Exception as e:
                err = str(e)
            oks = [None] * world
            dist.all_gather_object(oks, err, group=group)
            if any(oks):
                raise RuntimeError("in-library exchange unavailable on rank(s) %s: %s"
                                   % ([r for r, e in enumerate(oks) if e], next(e for e in oks if e)))
            box = [uid if rank == 0 else None]
            dist.broadcast_object_list(box, src=0, group=group)
            unique_id = box[0]
        else:
            rank = layout.cell0.index(tile.cell0) if layout.num_tiles > 1 else 0
            world = layout.num_tiles
        assert world == layout.num_tiles
        self.rank, self.world = rank, world
        tile.comm_init(layout.cell0, layout.ncells, rank, mode, unique_id)

    def exchange_and_solve(self):
        self.tile.exchange()


class LocalLibExchange:
    """All tiles in this process on one GPU, exchange done inside libscythe_hip.so with the loopback transport
    (sx_comm_init_local / sx_exchange_local): the RCCL path's buffer geometry and offsets with copies instead of sends."""

    def __init__(self, layout: PatchLayout, tiles, mode):
        import ctypes as C
        from . import _lib as L
        self._L, self.n = L, len(tiles)
        self.hs = (C.c_void_p * self.n)(*[g._h for g in tiles])
        c0 = (C.c_int32 * self.n)(*layout.cell0)
        nc = (C.c_int32 * self.n)(*layout.ncells)
        from .model import EXCHANGE_MODES
        L.check(L.load().sx_comm_init_local(self.hs, self.n, c0, nc, EXCHANGE_MODES[mode]))

    def exchange_and_solve(self):
        self._L.check(self._L.load().sx_exchange_local(self.hs, self.n))


class ModelRun:
    """initialize_model + run_model state for one process (src/semiimplicit.jl:126-256)."""

    def __init__(self, model: ModelParameters, num_tiles=1, rank=None, device=None, use_dist=False, exchange="a2a",
                 split="reference", impl="torch", unique_id=None):
        """exchange: "a2a" = transposed solve over all-to-all, "iface" = interface-only solve (tile-local solves, all-to-all of
        10 rows per tile around a small reduced system: least traffic, shortest recurrence), "gather" = the reference's
        protocol (halo chain + gather of owned rows + redundant patch solve on every tile), "auto" = "iface" where every tile
        has at least 9 cells, else "a2a".
        impl (use_dist only): "lib" = RCCL calls inside libscythe_hip.so on the tile's stream (sx_exchange; also valid with
        ONE tile, where every send is a send to self - the one-GPU self-test of that code path), "torch" =
        torch.distributed collectives on device tensors (also what the gloo rehearsals use)."""
        self.model = model
        patch = model.grid_params
        self.patch = patch
        self.num_tiles = num_tiles
        self.layout = PatchLayout(patch, num_tiles, split=split)
        if exchange == "auto":      # the interface-only solve where every tile is large enough for it (6 free coefficients: >= 9 cells
            exchange = "iface" if num_tiles > 1 and min(self.layout.ncells) >= 9 else "a2a"          # covers every boundary condition)
        self.use_dist = use_dist
        if use_dist:
            t = rank
            self.tiles = [Grid(patch, model, self.layout.cell0[t], self.layout.ncells[t], t + 2)]
            self.tile_ids = [t]
        else:
            self.tiles = [Grid(patch, model, self.layout.cell0[t], self.layout.ncells[t], t + 2)
                          for t in range(num_tiles)]
            self.tile_ids = list(range(num_tiles))
        self.exchange = None
        self.exchange_kind = exchange if num_tiles > 1 else "none"
        self.impl = impl if use_dist else "local"
        self._bind_streams(device)
        if use_dist and impl == "lib":
            self.exchange_kind = exchange
            self.exchange = LibExchange(self.layout, self.tiles[0], exchange, unique_id=unique_id)
        elif not use_dist and impl == "lib" and num_tiles > 1:
            self.impl = "lib"
            self.exchange = LocalLibExchange(self.layout, self.tiles, exchange)
        elif num_tiles > 1:
            if exchange in ("a2a", "iface"):
                self.exchange = (DistA2AExchange(self.layout, self.tiles[0], device, kind=exchange) if use_dist
                                 else LocalA2AExchange(self.layout, self.tiles, device, kind=exchange))
            elif exchange == "gather":
                self.exchange = (DistExchange(self.layout, self.tiles[0], device) if use_dist
                                 else LocalExchange(self.layout, self.tiles, device))
            else:
                raise ValueError("exchange must be 'a2a', 'iface' or 'gather'")
        self.t = 0
        self._ab0 = 0               # the step count at which the Adams-Bashforth start-up began: not 0 only in a run that regrid made
        self._device = device
        self._ring_axes = None      # azimuthal_mean's (r, z) axes, formed on first use
        self._points = None         # the local tiles' gridpoints [n, n_coord] in tile order (extrema's rows), formed on first use
        self._parcels = False       # set_parcels attached a parcel set: step() moves it
        self._stats = None          # set_statistics attached a statistics set: dict(source, every, key); step() samples it

    def _bind_streams(self, device):
        """Kernels of a tile run on ITS stream; torch's collectives order themselves against torch's CURRENT stream.  Hand
        that stream to the library so that both see one queue (with the default stream this is stream 0, as before)."""
        self._stream = None
        try:
            torch = _torch()
            if device is not None and torch.cuda.is_available():
                self._stream = torch.cuda.current_stream(device).cuda_stream
                for g in self.tiles:
                    g.set_stream(self._stream)
        except ImportError:
            pass

    def _check_stream(self):
        # every implementation but the in-library one issues torch operations (collectives, or the copies of the Local*
        # exchanges) on torch's CURRENT stream: the tiles' kernels must follow it
        if self._stream is not None and self.impl != "lib":
            cur = _torch().cuda.current_stream().cuda_stream
            if cur != self._stream:          # the caller entered a torch.cuda.stream(...) context: follow it
                self._stream = cur
                for g in self.tiles:
                    g.set_stream(cur)

    def tile_points(self, t):
        return self.tiles[self.tile_ids.index(t)].N

    def set_initial_conditions(self, values_by_tile):
        """read_physical_grid + spectralTransform!(patch) + first splineTransform! (:134-136, :233-237)."""
        for g, v in zip(self.tiles, values_by_tile):
            g.set_physical_values(v)
            g.spectralTransform_()
        self._exchange_and_solve()

    def _exchange_and_solve(self):
        self._check_stream()
        if self.impl == "lib":
            self.exchange.exchange_and_solve()
            return
        if self.exchange_kind in ("a2a", "iface"):
            self.exchange.exchange_and_solve()
            return
        if self.exchange is not None:
            self.exchange.exchange()
        for g in self.tiles:
            g.splineTransform_()

    def step(self):
        """One pass of model_loop's body (src/semiimplicit.jl:268-297) without the output branch."""
        self.t += 1
        if self._parcels:
            # the parcels move with the A of time n: their kernel goes on the tile's stream BEFORE the step, whose banded solve - the
            # only writer of A, on that same stream - therefore follows it; with SX_OVERLAP=1 the second stream forks after it and
            # never writes A
            self._check_stream()
            self.tiles[0].advance_parcels(self.model.ts)
        if self.num_tiles == 1 and self.exchange is None:
            self._check_stream()
            self.tiles[0].step(self.t - self._ab0)          # sx_step = sx_advance + sx_spline_transform (one hipGraph launch with SX_GRAPH=1)
        else:
            for g in self.tiles:
                g.advance(self.t - self._ab0)
            self._exchange_and_solve()
        if self._stats is not None and self.t % self._stats["every"] == 0:
            # the sample goes on each tile's stream AFTER the step: var_np1 is then the state of time t, and the next step's first
            # writer of var_np1 or `physical` is enqueued on that same stream behind it
            self._sample_statistics(self.t * self.model.ts, self._stats["every"] * self.model.ts)

    def _sample_statistics(self, time, weight):
        self._check_stream()
        for g in self.tiles:
            if self._stats["source"] == "physical":
                g.tileTransform_()
            g.accumulate_statistics(time, weight)

    def set_statistics(self, outputs, source="state", every=1, include_initial=True, ops=None, key=""):
        """Attach a statistics set to every local tile (Grid.set_statistics): from now on step() takes a sample AFTER every
        `every`-th step (t % every == 0) with time = t ts and weight = every ts, on each tile's stream and without a
        synchronisation.  include_initial takes the state as it stands into the extrema with weight 0 (time = t ts), which gives it
        no time weight.  source="state" reads var_np1 and costs nothing but the kernel; source="physical" runs tileTransform! on
        the tile before each sample, at that cadence only: one inverse transform per sample, which writes `physical` alone - the
        step rebuilds `physical` from the A coefficients before it reads it, so the model's evolution cannot change.  An empty
        `outputs` detaches the set."""
        if int(every) < 1:
            raise ValueError("every must be at least 1")
        for g in self.tiles:
            g.set_statistics(outputs, source, ops)
        if self.tiles[0].describe_statistics() is None:
            self._stats = None
            return
        self._stats = dict(source=source, every=int(every), key=str(key))
        if include_initial:
            self._sample_statistics(self.t * self.model.ts, 0.0)

    def statistics(self):
        """The statistics of the local tiles concatenated in tile order: the rows of gridpoints() (Grid.statistics)"""
        if self._stats is None:
            raise ValueError("statistics: no statistics set is attached (set_statistics)")
        self._check_stream()
        return Statistics.concatenate([g.statistics() for g in self._tiles_in_order()])

    def reset_statistics(self):
        """Empty the accumulators and counters of every local tile; the set stays attached (windowed means, hourly totals)"""
        for g in self.tiles:
            g.reset_statistics()

    def wind_swath(self, u, v, every=1):
        """The maximum-wind swath: the largest speed sqrt(u^2 + v^2) every gridpoint has seen, and when.  The first call attaches
        the set - MAX of u^2 + v^2 on var_np1, the state as it stands included - and every call returns Swath(speed [N], time [N],
        samples) over gridpoints()' rows; the square root is taken on the host.  A run holds ONE statistics set: this replaces
        another one."""
        key = "wind_swath:%s:%s" % (u, v)
        if self._stats is None or self._stats["key"] != key:
            self.set_statistics([("max", [(1.0, 0, [(u, ""), (u, "")]), (1.0, 0, [(v, ""), (v, "")])])], "state", every, True, key=key)
        st = self.statistics()
        return Swath(np.sqrt(st.value[:, 0]), st.time[:, 0].copy(), st.samples)

    def accumulated(self, var, every=1):
        """The time integral of variable `var` (rain rate -> rain, a flux -> its total).  The first call attaches the set - SUM of
        var on var_np1, weight every ts per sample - and every call returns (total [N], elapsed) over gridpoints()' rows.  A run
        holds ONE statistics set: this replaces another one."""
        key = "accumulated:%s" % (var,)
        if self._stats is None or self._stats["key"] != key:
            self.set_statistics([("sum", [(1.0, 0, [(var, "")])])], "state", every, False, key=key)
        st = self.statistics()
        return st.value[:, 0].copy(), st.elapsed

    def physical(self):
        """tileTransform! on every local tile; returns the concatenated physical array."""
        out = []
        for g in self.tiles:
            g.tileTransform_()
            out.append(g.physical)
        return np.concatenate(out, axis=0)

    def evaluate(self, points, all_k=False, k_band=None):
        """Grid.evaluate over the local tiles: every point goes to the local tile that contains its radius (a shared edge to the
        lower tile).  Returns (values [n, V, D], held [n] bool): held marks the points this process holds; the rows of the others
        are zero (write_output's convention: each process deals with its local tiles)."""
        patch = self.patch
        nco = len(patch.geometry)
        p = np.asarray(points, dtype=np.float64)
        p = p.reshape(-1, nco) if p.ndim != 2 else p
        g0 = self.tiles[0]
        out = np.zeros((p.shape[0], g0.V, g0.D), order="F")
        held = np.zeros(p.shape[0], dtype=bool)
        DX = (patch.xmax - patch.xmin) / patch.num_cells
        for t, g in sorted(zip(self.tile_ids, self.tiles)):
            c0, n = self.layout.cell0[t], self.layout.ncells[t]
            lo = patch.xmin if c0 == 0 else patch.xmin + c0 * DX                      # the extent sx_evaluate accepts
            hi = patch.xmax if c0 + n == patch.num_cells else patch.xmin + (c0 + n) * DX
            sel = np.nonzero((p[:, 0] >= lo) & (p[:, 0] <= hi) & ~held)[0]
            if len(sel):
                out[sel] = g.evaluate(p[sel], all_k, k_band)
                held[sel] = True
        return out, held

    def set_parcels(self, points, velocity):
        """Attach Lagrangian parcels to the run (Grid.set_parcels): from now on step() moves them with the model's time step, from the
        A coefficients of time n, before the step rewrites A.  One-tile patches only: a parcel that crosses a tile edge would have
        to be handed to the neighbour, which is not implemented."""
        if self.num_tiles > 1:
            raise ValueError("set_parcels: one-tile patches only (num_tiles = %d): parcels are not handed across tiles" % self.num_tiles)
        self.tiles[0].set_parcels(points, velocity)
        self._parcels = self.tiles[0].n_parcels > 0

    def parcels(self):
        """(positions, velocity, status) of the run's parcels (Grid.parcels)"""
        return self.tiles[0].parcels()

    def harmonics(self, radii, heights=None, all_k=False, slots=("u",)):
        """Grid.harmonics over the local tiles: every radius goes to the local tile that contains it (a shared edge to the lower
        tile, as in evaluate).  Returns (values [n_r, n_z, kDim + 1, V, n_slots] complex, held [n_r] bool); the rows of radii no
        local tile holds are zero."""
        patch = self.patch
        r = np.asarray(radii, dtype=np.float64).reshape(-1)
        g0 = self.tiles[0]
        n_z = 1 if heights is None else np.asarray(heights).size
        n_slots = len(set(slots))                                  # Grid.harmonics refuses what is no set of slot names
        out = np.zeros((len(r), n_z, int(g0.dims.kDim) + 1, g0.V, n_slots), dtype=np.complex128)
        held = np.zeros(len(r), dtype=bool)
        DX = (patch.xmax - patch.xmin) / patch.num_cells
        for t, g in sorted(zip(self.tile_ids, self.tiles)):
            c0, n = self.layout.cell0[t], self.layout.ncells[t]
            lo = patch.xmin if c0 == 0 else patch.xmin + c0 * DX
            hi = patch.xmax if c0 + n == patch.num_cells else patch.xmin + (c0 + n) * DX
            sel = np.nonzero((r >= lo) & (r <= hi) & ~held)[0]
            if len(sel):
                out[sel] = g.harmonics(r[sel], heights, all_k, slots)
                held[sel] = True
        return out, held

    # the wind variables (u, v) of the equation sets that have a horizontal wind by name
    _WIND = {"Oneway_ShallowWater_Slab": ("u", "v"), "Twoway_ShallowWater_Slab": ("u", "v"), "LinearShallowWaterRL": ("u", "v")}

    def _invert_wind(self, kind, u, v, alpha, into, var):
        if self.num_tiles > 1:
            raise ValueError("%s: one-tile patches only (num_tiles = %d)" % (kind, self.num_tiles))
        if u is None or v is None:
            if self.model.equation_set not in self._WIND:
                raise ValueError("%s: name the wind variables u and v of equation set %r" % (kind, self.model.equation_set))
            u, v = self._WIND[self.model.equation_set]
        self._check_stream()
        return self.tiles[0].invert((kind, u, v), alpha, into, var)

    def streamfunction(self, u=None, v=None, alpha=0.0, into=None, var=1, rhs=None):
        """The streamfunction psi of the wind, lap psi = vorticity, solved on the device from the A coefficients of time n
        (Grid.invert): returns the Grid that holds psi (a cached one-variable companion unless `into` names one; psi = 0 at the outer
        edge by default).  The rotational wind is (-psi_l / r, psi_r).  u, v: variable names or 1-based indices; the slab and linear
        shallow-water sets know theirs.  rhs=<terms> solves lap psi = that field program of `physical` instead - an arbitrary
        forcing, projected first (project).  One-tile RL / RLZ patches."""
        if rhs is not None:
            self._one_tile("streamfunction")
            self._check_stream()
            self.tiles[0].tileTransform_()
            return self.tiles[0].invert(rhs, alpha, into, var)
        return self._invert_wind("vorticity", u, v, alpha, into, var)

    def velocity_potential(self, u=None, v=None, alpha=0.0, into=None, var=1):
        """The velocity potential chi of the wind, lap chi = divergence (Grid.invert); the divergent wind is (chi_r, chi_l / r).
        Arguments as for streamfunction.  With into=None it shares streamfunction's companion: pass a Grid of your own to keep both."""
        return self._invert_wind("divergence", u, v, alpha, into, var)

    def antiderivative(self, var, axis="r", origin="low", weight_r=False, into=None, var_dst=1):
        """The integral of variable `var` of time n up to a point along r or z, on the device (Grid.antiderivative): returns the
        Grid that holds it (a cached one-variable companion unless `into` names one), to be sampled like any field.  One-tile
        patches."""
        if self.num_tiles > 1:
            raise ValueError("antiderivative: one-tile patches only (num_tiles = %d)" % self.num_tiles)
        self._check_stream()
        if isinstance(var, (tuple, list)):          # a field program of `physical`, projected first (Grid.antiderivative)
            self.tiles[0].tileTransform_()
        return self.tiles[0].antiderivative(var, axis, origin, weight_r, into, var_dst)

    def project(self, outputs, names=None, source="physical", bcs=None, transform=False):
        """Derived fields as spectral variables (Grid.project): every output - a list of (coef, r_power, [(var, slot), ...]) terms; a
        list of them, or a dict name -> terms such as field_programs(model) gives - becomes one variable of a companion Grid, which
        is returned: evaluate, harmonics, spectrum, vortex_harmonics, invert, antiderivative and refine_extremum then apply to the
        vorticity, a flux or the kinetic energy as to any variable.  The companion is made on first use and kept per (names,
        conditions); bcs are companion_grid's conditions (default: R0 everywhere).  source="physical" runs tileTransform! on the tile
        first; source="state" reads var_np1.  transform=True also runs the companion's tileTransform!, so that its `physical` holds
        the derived fields and their derivatives at the gridpoints.  One-tile patches."""
        self._one_tile("project")
        if isinstance(outputs, dict):
            names, outputs = list(outputs) if names is None else list(names), list(outputs.values())
        names = ["f%d" % (o + 1) for o in range(len(outputs))] if names is None else list(names)
        if len(names) != len(outputs):
            raise ValueError("project: %d names for %d outputs" % (len(names), len(outputs)))
        self._check_stream()
        tile = self.tiles[0]
        if source == "physical":
            tile.tileTransform_()
        into = tile.project(program_of_outputs(outputs), tile.project_companion(names, **(bcs or {})), source)
        if transform:
            into.tileTransform_()
        return into

    def derive(self, outputs, names=None, source="physical", bcs=None):
        """Nonlinear derived fields as spectral variables (Grid.derive): every output - a term list or an expression as
        pack_function_program reads them; a list of them, or a dict name -> output such as function_programs(model) or
        thermo_programs(model) give - becomes one variable of a companion Grid, which is returned, to be sampled, scanned and
        inverted like any state: the speed, a potential vorticity, temperature, pressure, theta_e.  Companion, bcs and source as
        for project.  One-tile patches."""
        self._one_tile("derive")
        if not isinstance(outputs, dict):
            outputs = dict(zip(["f%d" % (o + 1) for o in range(len(outputs))] if names is None else list(names), outputs))
        elif names is not None:
            outputs = {n: outputs[n] for n in names}
        self._check_stream()
        tile = self.tiles[0]
        if source == "physical":
            tile.tileTransform_()
        return tile.derive(outputs, tile.project_companion(list(outputs), **(bcs or {})), source)

    def freezing_level(self, columns):
        """The lowest height at which the temperature crosses 273.15 K in every column r[, lambda] (Euler_test / rainfall_test):
        derive of thermo_programs' T, then height_where on the companion.  ndarray [n_cols], NaN where a column has no crossing."""
        return self.height_where([(0, 1.0, 0, [("T", "")])], 273.15, columns, grid=self.derive({"T": thermo_programs(self.model)["T"]}))

    def minimum_pressure(self):
        """(p [hPa], gridpoint [n_coord]) of the lowest pressure on the grid (Euler_test / rainfall_test): derive of thermo_programs'
        p, then Grid.extrema on the companion's state."""
        val, idx = self.derive({"p": thermo_programs(self.model)["p"]}).extrema([(0, 1.0, 0, [("p", "")])], "domain", "state")
        return float(val[0, 0]), self.gridpoints()[int(idx[0, 0])].copy()

    def column_integral(self, var):
        """int_{zmin}^{zmax} f dz of variable `var` in every column of the grid: (points [columns, n_coord - 1] - r[, lambda] of the
        columns in gridpoint order -, values [columns]); the vertical antiderivative sampled at zmax with the wavenumber cut of each
        ring (precipitable water, the mass of a column).  One-tile RZ / RLZ patches."""
        F = self.antiderivative(var, "z")
        pts = self.gridpoints()
        top = pts[self.patch.zDim - 1::self.patch.zDim]
        return top[:, :-1].copy(), F.evaluate(top)[:, 0, 0]

    def inside_radius(self, var, radii=None):
        """int_{xmin}^{r} f s ds of the azimuthal mean (wavenumber 0) of variable `var` at the radii given (default: the rings'):
        (r [n], values [n] or [n, zDim] on a grid with a vertical, at the levels).  2 pi times it is the integral over the disc: the
        circulation of a vorticity, the mass of a depth.  One-tile patches."""
        F = self.antiderivative(var, "r", weight_r=True)
        if radii is None:
            r = self.gridpoints()[:, 0]
            radii = r[np.concatenate([[True], r[1:] != r[:-1]])]
        radii = np.atleast_1d(np.asarray(radii, dtype=np.float64))
        geo = self.patch.geometry
        z = self.gridpoints()[:self.patch.zDim, -1] if "Z" in geo else np.zeros(1)
        cols = [np.repeat(radii, len(z))] + ([np.zeros(len(radii) * len(z))] if "L" in geo else []) + ([np.tile(z, len(radii))] if "Z" in geo else [])
        val = F.evaluate(np.stack(cols, axis=1), k_band=(0, 0) if "L" in geo else None)[:, 0, 0].reshape(len(radii), len(z))
        return radii, (val if "Z" in geo else val[:, 0])

    def _tiles_in_order(self):
        """the local tiles by tile number"""
        return [g for _, g in sorted(zip(self.tile_ids, self.tiles), key=lambda tg: tg[0])]

    def integrate(self, terms, source="physical"):
        """Domain integrals of field products over the local tiles (Grid.reduce, kind="domain"): ndarray [n_out], the tile results
        summed in tile order.  source="physical" runs tileTransform! on every local tile first; source="state" reads var_np1 and
        costs no transform.  With one process per GPU every rank returns its own tiles' share (evaluate's convention: no
        collective is added)."""
        total = np.zeros(max((int(term[0]) for term in terms), default=-1) + 1)
        for g in self._tiles_in_order():
            if source == "physical":
                g.tileTransform_()
            total = total + g.reduce(terms, "domain", source)
        return total

    def azimuthal_mean(self, terms, source="physical"):
        """Azimuthal means of field products over the local tiles (Grid.reduce, kind="azimuth"): (r [rings], z [zDim] or [0.0]
        without a vertical, mean [rings, zDim, n_out]), the rings of the local tiles concatenated in tile order."""
        if self._ring_axes is None:       # the rings' radii and the levels: functions of the grid, formed once
            rs, z = [], np.zeros(1)
            for g in self._tiles_in_order():
                pts = getGridpoints(g)
                pts = pts.reshape(len(pts), -1)
                r = pts[:, 0]
                rs.append(r[np.concatenate([[True], r[1:] != r[:-1]])])      # ring-major points: a ring's radius is one double
                if "Z" in self.patch.geometry:
                    z = pts[:self.patch.zDim, -1].copy()
            self._ring_axes = (np.concatenate(rs), z)
        means = []
        for g in self._tiles_in_order():
            if source == "physical":
                g.tileTransform_()
            means.append(g.reduce(terms, "azimuth", source))
        rs, z = self._ring_axes
        return rs.copy(), z.copy(), np.concatenate(means, axis=0)

    def gridpoints(self):
        """The gridpoints of the local tiles in tile order, [n, n_coord]: the rows extrema's idx names (formed once and kept)"""
        if self._points is None:
            pts = [getGridpoints(g) for g in self._tiles_in_order()]
            self._points = np.concatenate([p.reshape(len(p), -1) for p in pts], axis=0)
        return self._points

    def extrema(self, terms, kind="domain", source="physical"):
        """Minimum and maximum of field programs over the local tiles, with their locations (Grid.extrema): (val, idx), idx a row
        of self.gridpoints().  kind="domain": [2, n_out], the tile results folded in tile order with Grid.extrema's own order
        (value, then the lower row; a NaN wins).  kind="azimuth": [2, rings, levels, n_out], the rings of the local tiles
        concatenated in tile order.  source="physical" runs tileTransform! on every local tile first."""
        vals, idxs, off = [], [], 0
        for g in self._tiles_in_order():
            if source == "physical":
                g.tileTransform_()
            v, i = g.extrema(terms, kind, source)
            vals.append(v)
            idxs.append(i + off)
            off += g.N
        if kind != "domain":
            return np.concatenate(vals, axis=1), np.concatenate(idxs, axis=1)
        val, idx = vals[0].copy(), idxs[0].copy()
        for v, i in zip(vals[1:], idxs[1:]):       # later tiles hold higher rows: they win only when strictly better, or NaN first
            for w, better in ((0, v[0] < val[0]), (1, v[1] > val[1])):
                take = (better | np.isnan(v[w])) & ~np.isnan(val[w])
                val[w], idx[w] = np.where(take, v[w], val[w]), np.where(take, i[w], idx[w])
        return val, idx

    def distribution(self, terms, edges, kind="domain", source="physical"):
        """Histogram of a field program over the local tiles (Grid.distribution): Distribution(count, measure, sums, edges), the
        counts of the tiles added exactly and their sums in tile order.  source="physical" runs tileTransform! on every local
        tile first."""
        total = None
        for g in self._tiles_in_order():
            if source == "physical":
                g.tileTransform_()
            d = g.distribution(terms, edges, kind, source)
            total = d if total is None else Distribution(total.count + d.count, total.measure + d.measure, total.sums + d.sums, d.edges)
        return total

    def cfad(self, var_or_terms, edges, normalize=True, source="physical"):
        """Contoured frequency-by-altitude diagram of a variable (name or 1-based index) or of a one-output program: Cfad(frac
        [n_bins, zDim], under [zDim], over [zDim], nan [zDim], area [zDim], edges): per level the fraction of the horizontal area
        whose value lies in each bin, and the fractions below edges[0], at or above edges[-1] and NaN - every column of frac sums
        to 1 with its three outside fractions.  normalize=False returns the areas themselves.  One column on a grid without a
        vertical."""
        terms = var_or_terms if isinstance(var_or_terms, (list, tuple)) else [(0, 1.0, 0, [(var_or_terms, "")])]
        d = self.distribution(terms, edges, "level", source)
        area = d.measure.sum(axis=0)
        m = d.measure / area[None, :] if normalize else d.measure
        return Cfad(m[1:-2].copy(), m[0].copy(), m[-2].copy(), m[-1].copy(), area, d.edges)

    def exceedance(self, terms, thresholds, integrand=None, source="physical"):
        """Measure, and optionally integral, of {q >= c} for each of up to 65 increasing thresholds c, q the one-output program
        `terms`: ONE Grid.distribution call per tile with the thresholds as edges, cumulative sums from the top slot down, NaN
        points excluded.  integrand: the terms of one integrand (their `out` is ignored).  Returns Exceedance(thresholds, measure
        [n], integral [n] or None): area on R / RL grids, volume with a vertical."""
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        edges = thr if len(thr) > 1 else np.array([thr[0], np.nextafter(thr[0], np.inf)])
        prog = [(0, c, p, f) for _, c, p, f in terms] + [(1, c, p, f) for _, c, p, f in (integrand or [])]
        d = self.distribution(prog, edges, "domain", source)
        top_down = np.cumsum(d.sums[-2:0:-1, :, 0], axis=0)[::-1]           # row i: slots i + 1 .. overflow
        top_down = top_down[:len(thr)] if len(thr) > 1 else top_down[:1]
        return Exceedance(thr, top_down[:, 0].copy(), top_down[:, 1].copy() if integrand else None)

    def integrated_kinetic_energy(self, u, v, thresholds, density=1.0, source="physical"):
        """Integrated kinetic energy above wind-speed thresholds (IKE at 18 / 26 / 33 m/s): q = u^2 + v^2 is binned at
        thresholds^2 and 1/2 density (u^2 + v^2) integrated over {speed >= threshold} (exceedance).  Returns Exceedance(thresholds,
        measure, integral)."""
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        q = [(0, 1.0, 0, [(u, ""), (u, "")]), (0, 1.0, 0, [(v, ""), (v, "")])]
        ke = [(1, 0.5 * float(density), 0, [(u, ""), (u, "")]), (1, 0.5 * float(density), 0, [(v, ""), (v, "")])]
        res = self.exceedance(q, thr ** 2, ke, source)
        return Exceedance(thr, res.measure, res.integral)

    def quantile(self, terms, p, tol=1e-6, max_passes=8, source="physical"):
        """The measure-weighted p-quantile of the one-output program `terms`, bracketed by repeated histograms: Quantile(lo, hi,
        passes, nan_count, measure) with measure{q < lo} <= p M < measure{q < hi}, M the measure of the non-NaN points.  The first
        edges are 64 uniform bins from the minimum to one ulp above the maximum (extrema); every later pass re-bins the slot that
        holds p M, until hi - lo <= tol (max - min), the slot holds one point, the edges can no longer be made strictly increasing
        or max_passes are taken.  NaN points are counted, not ranked (with a NaN present the first edges span all doubles in
        decades instead)."""
        val, _ = self.extrema(terms, "domain", source)
        mn, mx = float(val[0, 0]), float(val[1, 0])
        if np.isfinite(mn) and np.isfinite(mx):
            edges = np.linspace(mn, np.nextafter(mx, np.inf), 65)
            edges[0], edges[-1] = mn, np.nextafter(mx, np.inf)
            span = mx - mn
        else:
            pw = 10.0 ** np.linspace(-300.0, 300.0, 32)
            edges, span = np.concatenate([-pw[::-1], [0.0], pw]), 0.0
        lo = hi = np.nan
        passes = nan_count = 0
        M = 0.0
        while passes < max_passes and (np.diff(edges) > 0).all() and np.isfinite(edges).all():
            d = self.distribution(terms, edges, "domain", source)
            passes += 1
            m, c = d.measure[:-1, 0], d.count[:-1, 0]
            cum = np.concatenate([[0.0], np.cumsum(m)])                      # cum[k] = measure{q in a slot below k}
            if passes == 1:
                M, nan_count = float(cum[-1]), int(d.count[-1, 0])
            inside = np.nonzero((cum[:-1] <= p * M) & (p * M < cum[1:]))[0]
            k = int(inside[0]) if len(inside) else int(np.nonzero(c)[0][-1]) if c.any() else 0
            if k < 1 or k > len(edges) - 1:                                  # outside the edges: the bracket of the pass before stands
                break
            lo, hi = float(edges[k - 1]), float(edges[k])
            if hi - lo <= tol * span or c[k] == 1:
                break
            edges = np.linspace(lo, hi, 65)
            edges[0], edges[-1] = lo, hi
        return Quantile(lo, hi, passes, nan_count, M)

    def _one_tile(self, what):
        if self.num_tiles > 1:
            raise ValueError("%s: one-tile patches only (num_tiles = %d)" % (what, self.num_tiles))
        self._check_stream()
        return self.tiles[0]

    def locate(self, var, want="min", source="state", refine=True):
        """The one-call centre or peak: one domain scan of variable `var` (name or 1-based index) for its minimum (want="min") or
        maximum ("max"), then the refinement of that gridpoint to the stationary point of the continuous state
        (Grid.refine_extremum) with every coordinate free - z frozen when the gridpoint lies on the lowest or highest level.
        Returns Located(pos [n_coord], value, status): status as refine_extremum gives it; refine=False returns the gridpoint, its
        value and status 0.  source="state" scans var_np1 (no transform), "physical" runs tileTransform! first.  One-tile patches."""
        if want not in ("min", "max"):
            raise ValueError("want must be 'min' or 'max'")
        g = self._one_tile("locate")
        val, idx = self.extrema([(0, 1.0, 0, [(var, "")])], "domain", source)
        w = 0 if want == "min" else 1
        row = int(idx[w, 0])
        start = self.gridpoints()[row]
        if not refine:
            return Located(start.copy(), float(val[w, 0]), 0)
        free = self.patch.geometry.lower()
        if "z" in free and row % self.patch.zDim in (0, self.patch.zDim - 1):
            free = free.replace("z", "")
        res = g.refine_extremum(var, start[None, :], want, free)
        return Located(res.pos[0].copy(), float(res.value[0]), int(res.status[0]))

    def regrid(self, gp_new, centre=None, outside="refuse", fill=None):
        """The run continued on another grid (Grid.regrid): a new ModelRun on `gp_new` with the same model and the same variables by
        name, its state the continuous state of this run at gp_new's gridpoints - a finer or coarser mesh, other levels, a cropped or
        extended domain, or with centre=(x0, y0) a grid about another axis (RL / RLZ).  The step count t and with it the time are
        carried; the Adams-Bashforth start-up is restarted (the next steps are Euler, AB2, AB3: the tendency history belongs to the old
        grid), and `physical` is refreshed by one tileTransform!.  outside, fill: as for Grid.regrid; the number of columns filled is
        the new run's n_outside.  Parcels and statistics are not carried: a run with either attached raises ValueError (detach them,
        or read them out first).  This run is left as it is.  One-tile patches."""
        src = self._one_tile("regrid")
        if self._parcels or self._stats is not None:
            raise ValueError("regrid: attached parcels and statistics are not carried onto another grid (detach them first)")
        keep_ref = self.model.ref_state if not self.model.ref_state_file else None      # a file's reference state is rebuilt for the new levels
        new = ModelRun(dataclasses.replace(self.model, grid_params=gp_new, ref_state=keep_ref), num_tiles=1, device=self._device)
        try:
            new.n_outside = src.regrid(new.tiles[0], centre, None, outside, fill)
            new.tiles[0].tileTransform_()
        except Exception:
            new.close()
            raise
        new.t = new._ab0 = self.t
        return new

    def recentre(self, centre=None, var=None, want="min", **kw):
        """regrid onto this run's own GridParameters about `centre` (default: self.locate(var, want) - the vortex centre): the model
        follows its vortex, and every ring truncation sits about the axis again.  kw: regrid's outside and fill; with outside="fill"
        and no fill every variable takes its azimuthal mean at this grid's outermost ring (azimuthal_mean of the state, averaged over
        the levels).  Returns the new ModelRun.  One-tile RL / RLZ patches."""
        self._one_tile("recentre")
        if "L" not in self.patch.geometry:
            raise ValueError("recentre: RL and RLZ grids only")
        if centre is None:
            if var is None:
                raise ValueError("recentre: give a centre, or the variable whose extremum is the centre")
            pos = self.locate(var, want).pos
            centre = (pos[0] * np.cos(pos[1]), pos[0] * np.sin(pos[1]))
        if kw.get("outside") == "fill" and kw.get("fill") is None:
            names = self.patch.var_names()
            _, _, mean = self.azimuthal_mean([(o, 1.0, 0, [(n, "")]) for o, n in enumerate(names)], "state")
            kw["fill"] = mean[-1].mean(axis=0)
        return self.regrid(self.patch, centre, **kw)

    def radius_of_maximum(self, var, level=None, source="state"):
        """The radius of the maximum of variable `var` (the radius of maximum wind for the tangential wind): the azimuth kind's
        maxima over lambda at every ring (Grid.extrema) on `level` (0-based; None: the level that holds the largest), the ring of
        the largest, then the refinement along that ray - lambda and z frozen at the gridpoint's (Grid.refine_extremum).
        Returns Located(pos [n_coord], value, status); pos[0] is the radius.  One-tile patches."""
        g = self._one_tile("radius_of_maximum")
        val, idx = self.extrema([(0, 1.0, 0, [(var, "")])], "azimuth", source)
        mx = val[1, :, :, 0] if level is None else val[1, :, int(level):int(level) + 1, 0]
        ring, lev = np.unravel_index(int(np.argmax(mx)), mx.shape)
        row = int(idx[1, ring, lev if level is None else int(level), 0])
        start = self.gridpoints()[row]
        res = g.refine_extremum(var, start[None, :], "max", "r")
        return Located(res.pos[0].copy(), float(res.value[0]), int(res.status[0]))

    def vortex_profile(self, wind=None, centre=None, radii=None, heights=None, kmax=2, motion=None):
        """The wind profile of the vortex about ITS centre (Grid.vortex_harmonics): wind = (u, v), the grid's radial and tangential
        wind by name or 1-based index (the slab and linear shallow-water sets know theirs); centre = (x0, y0), Cartesian, default
        locate("h", "min") - the refined minimum of h; radii from the centre (default: the patch's ring radii that fit between the
        centre and the outer edge); heights as for harmonics.  Returns VortexProfile(centre, radii, radial [n_rho, n_z], tangential
        [n_rho, n_z]: the azimuthal means Re c_0 about the centre; wave1, wave2 [2, n_rho, n_z]: the amplitudes 2 |c_k| of the
        radial and the tangential wind (NaN above kmax); status [n_rho]: 1 where the circle leaves the patch and the row is NaN).
        With motion = (cx, cy) the storm motion is taken out of wave 1.  Reads the A coefficients as they stand; one-tile patches."""
        g = self._one_tile("vortex_profile")
        if wind is None:
            if self.model.equation_set not in self._WIND:
                raise ValueError("vortex_profile: name the wind variables (u, v) of equation set %r" % self.model.equation_set)
            wind = self._WIND[self.model.equation_set]
        if centre is None:
            pos = self.locate("h", "min").pos
            centre = (pos[0] * np.cos(pos[1]), pos[0] * np.sin(pos[1]))
        centre = np.asarray(centre, dtype=np.float64).reshape(-1)
        if radii is None:
            DX = (self.patch.xmax - self.patch.xmin) / self.patch.num_cells
            n = int(np.floor((self.patch.xmax - float(np.hypot(centre[0], centre[1]))) / DX))
            radii = DX * np.arange(max(n, 0) + 1)
        radii = np.asarray(radii, dtype=np.float64).reshape(-1)
        c, status = g.vortex_harmonics(centre, radii, heights, [("wind", wind[0], wind[1])], kmax=kmax, motion=motion)
        amp = [2.0 * np.abs(c[:, :, :, k]) if k <= kmax else np.full(c.shape[:3], np.nan) for k in (1, 2)]
        return VortexProfile(centre, radii, c[0, :, :, 0].real.copy(), c[1, :, :, 0].real.copy(), amp[0], amp[1], status)

    def radius_of_maximum_about(self, centre, radii, wind=None, height=None):
        """The radius of maximum wind about `centre` = (x0, y0): the largest azimuthal-mean tangential wind (Re c_0 of
        vortex_profile) among the given radii, at `height` on a grid with a vertical.  Returns (radius, value); circles that leave
        the patch do not take part.  One-tile patches."""
        p = self.vortex_profile(wind, centre, radii, None if height is None else [height], kmax=0)
        vt = np.where(p.status == 0, p.tangential[:, 0], -np.inf)
        if not np.isfinite(vt).any():
            raise ValueError("radius_of_maximum_about: no circle lies inside the patch")
        i = int(np.argmax(vt))
        return float(p.radii[i]), float(vt[i])

    def _rays(self, azimuths, height):
        """[n, n_coord - 1] ray coordinates lambda[, z] of the patch's geometry from azimuths and one height"""
        geo = self.patch.geometry
        lam = np.atleast_1d(np.asarray(azimuths if azimuths is not None else [0.0], dtype=np.float64))
        cols = [lam] if "L" in geo else []
        if "Z" in geo:
            if height is None:
                raise ValueError("a grid with a vertical needs a height")
            cols.append(np.full(len(lam), float(height)))
        elif height is not None:
            raise ValueError("the grid has no vertical: height must be None")
        return np.stack(cols, axis=1) if cols else np.zeros((len(lam), 0))

    def radius_where(self, terms, level, azimuths, height=None, which="outermost"):
        """The radius at which the one-output program `terms` (as for Grid.reduce) crosses `level` along the ray of every azimuth
        at `height` (Grid.crossings, up to 16 crossings per ray kept).  which="outermost" / "innermost": ndarray [n_azimuths], NaN
        where the ray has no crossing (or, outermost, more than 16); which="all": (radius [16, n_azimuths] outward, NaN-padded,
        dir of that shape, count [n_azimuths]).  Reads the A coefficients as they stand; one-tile patches."""
        if which not in ("outermost", "innermost", "all"):
            raise ValueError("which must be 'outermost', 'innermost' or 'all'")
        g = self._one_tile("radius_where")
        rays = self._rays(azimuths, height)
        res = g.crossings(terms, [level], rays if rays.shape[1] else len(rays), max_cross=16)
        rad, cnt = res.radius[:, 0, :], res.count[0]
        if which == "all":
            return rad, res.dir[:, 0, :], cnt
        if which == "innermost":
            return rad[0].copy()
        kept = (cnt >= 1) & (cnt <= 16)
        return np.where(kept, rad[np.clip(cnt - 1, 0, 15), np.arange(len(cnt))], np.nan)

    def wind_radii(self, u_var, v_var, thresholds, n_azimuths=360, height=None, quadrants=True):
        """Wind radii (R34 / R50 / R64 ...): for every threshold the radius of the outermost crossing along each of n_azimuths
        equally spaced rays at which the speed^2 = u^2 + v^2 of the wind (u_var, v_var) FALLS outward through threshold^2
        (Grid.crossings, the first 16 crossings of a ray).  Returns WindRadii(thresholds, azimuths [n], radii [n_thresholds, n] with
        NaN where a ray has no such crossing, quadrants [n_thresholds, 4] or None): the largest radius over the rays of the NE, SE,
        SW and NW quadrant (lambda in [0, pi/2), [3 pi/2, 2 pi), [pi, 3 pi/2), [pi/2, pi): lambda = 0 points east, counter-clockwise),
        NaN where no ray of the quadrant crosses.  One-tile patches."""
        g = self._one_tile("wind_radii")
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        n = int(n_azimuths)
        lam = 2.0 * np.pi * np.arange(n) / n
        rays = self._rays(lam, height)
        prog = [(0, 1.0, 0, [(u_var, ""), (u_var, "")]), (0, 1.0, 0, [(v_var, ""), (v_var, "")])]
        radii = np.full((len(thr), n), np.nan)
        for j0 in range(0, len(thr), 8):
            res = g.crossings(prog, thr[j0:j0 + 8] ** 2, rays if rays.shape[1] else n, max_cross=16)
            falling = np.where(res.dir == -1, res.radius, -np.inf)           # [16, levels, n], outward: the last falling one is the largest
            best = falling.max(axis=0)
            radii[j0:j0 + 8] = np.where(np.isfinite(best), best, np.nan)
        quad = None
        if quadrants:
            q = np.floor(lam / (np.pi / 2.0)).astype(int) % 4                # 0 NE, 1 NW, 2 SW, 3 SE
            quad = np.full((len(thr), 4), np.nan)
            for col, which in enumerate((0, 3, 2, 1)):
                sel = radii[:, q == which]
                ok = ~np.isnan(sel)
                if sel.shape[1]:
                    quad[:, col] = np.where(ok.any(axis=1), np.where(ok, sel, -np.inf).max(axis=1), np.nan)
        return WindRadii(thr, lam, radii, quad)

    @staticmethod
    def _pick_height(res, which, rising=None):
        """[n_cols] row index into res.height[:, 0, :] of the lowest / highest kept crossing (rising: among those with dir == +1,
        False: -1), -1 where the column has none"""
        hgt, dr = res.height[:, 0, :], res.dir[:, 0, :]
        ok = ~np.isnan(hgt) & (True if rising is None else dr == (1 if rising else -1))
        first = np.argmax(ok, axis=0)
        last = ok.shape[0] - 1 - np.argmax(ok[::-1], axis=0)
        return np.where(ok.any(axis=0), first if which == "lowest" else last, -1)

    def height_where(self, terms, level, columns, which="lowest", rising=None, grid=None):
        """The height at which the one-output program `terms` (as for Grid.reduce) crosses `level` in every column r[, lambda]
        (Grid.isosurface, up to 16 crossings per column kept): the vertical radius_where.  which="lowest" / "highest"; rising=True
        keeps the crossings where the program rises upward through the level, False those where it falls, None all.  Returns
        ndarray [n_cols], NaN where a column has no such crossing (or, highest, more than 16 crossings).  Reads the A coefficients
        as they stand; one-tile patches.  grid: a companion Grid (project, derive) whose variables the program names instead."""
        if which not in ("lowest", "highest"):
            raise ValueError("which must be 'lowest' or 'highest'")
        g = grid if grid is not None else self._one_tile("height_where")
        res = g.isosurface(terms, [level], columns, max_cross=16)
        k = self._pick_height(res, which, rising)
        out = np.where(k >= 0, res.height[np.maximum(k, 0), 0, np.arange(len(k))], np.nan)
        return np.where((which == "highest") & (res.count[0] > 16), np.nan, out)

    def on_surface(self, surface_terms, level, fields, columns, which="lowest"):
        """Fields on a surface: the height at which the one-output program `surface_terms` crosses `level` in every column
        (which="lowest" / "highest" crossing), and `fields` there - variable names (or 1-based indices) or term lists as for
        Grid.reduce (their `out` is ignored), which become the carried outputs of ONE Grid.isosurface call (at most 8).  Returns
        (height [n_cols], values [n_fields, n_cols]), NaN where a column has no crossing.  One-tile patches."""
        if which not in ("lowest", "highest"):
            raise ValueError("which must be 'lowest' or 'highest'")
        g = self._one_tile("on_surface")
        prog = [(0, c, p, f) for (_, c, p, f) in surface_terms]
        for o, fld in enumerate(fields):
            terms = [(0, 1.0, 0, [(fld, "")])] if isinstance(fld, (str, int, np.integer)) else fld
            prog += [(1 + o, c, p, f) for (_, c, p, f) in terms]
        res = g.isosurface(prog, [level], columns, carry=len(fields), max_cross=16)
        k = self._pick_height(res, which)
        cols = np.arange(len(k))
        none = (k < 0) | ((which == "highest") & (res.count[0] > 16))
        hgt = np.where(none, np.nan, res.height[np.maximum(k, 0), 0, cols])
        vals = np.zeros((len(fields), len(k)))
        if len(fields):
            vals = np.where(none[None, :], np.nan, res.carry[:, :, 0, :][:, np.maximum(k, 0), cols])
        return hgt, vals

    def spectrum(self, pairs, kind="ring"):
        """Azimuthal power and cross spectra over the local tiles (Grid.spectrum; reads A: no transform is run).  kind="domain":
        ndarray [kDim + 1, n_pairs], the tile results summed in tile order.  kind="ring": [kDim + 1, rings, n_pairs], the rings of
        the local tiles concatenated in tile order (azimuthal_mean's ring axis)."""
        parts = [g.spectrum(pairs, kind) for g in self._tiles_in_order()]
        if kind == "ring":
            return np.concatenate(parts, axis=1)
        total = np.zeros_like(parts[0])
        for p in parts:
            total = total + p
        return total

    def patch_spectral(self):
        """mtile.patchSpectral as the master pulls it from a worker for output (src/semiimplicit.jl:288-293): the patch's A
        coefficients [s_patch, V].  With the reference's protocol every tile holds the whole patch; with the transposed solve a
        tile only holds the rows it evaluates, so the patch array is assembled from every tile's OWNED rows (output cadence
        only; one process per GPU: gathered to rank 0, other ranks return None)."""
        if self.exchange_kind not in ("a2a", "iface"):
            return self.tiles[0].patchSpectral
        nb = self.layout.b_rDim
        parts = []
        for t, g in zip(self.tile_ids, self.tiles):
            # reference layout of one variable's column: s = (z-mode * n_blocks + block) * b_rDim + node, the node FASTEST
            a = g.patchSpectral.reshape(nb, -1, g.V, order="F")             # [node, z-mode x block, var]
            c0 = self.layout.cell0[t]
            parts.append((c0, np.ascontiguousarray(a[c0:c0 + self.layout.owned_rows(t)])))
        if self.use_dist:
            import torch.distributed as dist
            box = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
            dist.gather_object(parts, box, dst=0)
            if dist.get_rank() != 0:
                return None
            parts = [p for ps in box for p in ps]
        out = np.zeros((nb, parts[0][1].shape[1], parts[0][1].shape[2]))
        for c0, rows in parts:
            out[c0:c0 + rows.shape[0]] = rows
        return out.reshape(-1, out.shape[2], order="F")

    def synchronize(self):
        for g in self.tiles:
            g.synchronize()

    def save_checkpoint(self, path):
        """Restart file of the local tiles after step self.t (one .npz; with one process per GPU every rank writes its
        own path).  The reference restarts from a physical_out CSV only, i.e. with an Euler / AB2 start-up; this keeps
        the AB3 history so that the continued run is bit-identical to an uninterrupted one."""
        extra = {"tile%d" % i: g.get_state() for i, g in zip(self.tile_ids, self.tiles)}
        for i, g in zip(self.tile_ids, self.tiles):       # a parcel set travels with its tile; without one the file is what it always was
            blob = g.get_parcel_state()
            if blob is not None:
                extra["parcels%d" % i] = blob
        if self._stats is not None:                       # so does a statistics set, with the cadence it is sampled at
            for i, g in zip(self.tile_ids, self.tiles):
                extra["stats%d" % i] = g.get_statistics_state()
            extra["stats_every"], extra["stats_key"] = np.array(self._stats["every"]), np.array(self._stats["key"])
        np.savez(path, t=self.t, ab0=self._ab0, tile_ids=np.array(self.tile_ids), **extra)

    def load_checkpoint(self, path):
        with np.load(path) as z:
            if list(z["tile_ids"]) != list(self.tile_ids):
                raise ValueError("checkpoint holds tiles %s, this run holds %s" % (list(z["tile_ids"]), self.tile_ids))
            for i, g in zip(self.tile_ids, self.tiles):
                g.set_state(z["tile%d" % i])
                if "parcels%d" % i in z.files:
                    g.set_parcel_state(z["parcels%d" % i])
                else:
                    g.set_parcels(np.zeros((0, len(self.patch.geometry))), [None] * len(self.patch.geometry))
                if "stats%d" % i in z.files:
                    g.set_statistics_state(z["stats%d" % i])
                else:
                    g.set_statistics([])
            self._parcels = any(g.n_parcels > 0 for g in self.tiles)
            d = self.tiles[0].describe_statistics()
            self._stats = None if d is None else dict(source=d[0], every=int(z["stats_every"]), key=str(z["stats_key"]))
            self.t = int(z["t"])
            self._ab0 = int(z["ab0"]) if "ab0" in z.files else 0

    def close(self):
        for g in self.tiles:
            g.close()


def integrate_model(model: ModelParameters, num_tiles=1, verbose=False):
    """integrate_model(model) (src/Scythe.jl:37-62) on one GPU: initial conditions from CSV, time loop with
    output every output_interval, final output. Returns True like run_model."""
    from .io import read_physical_grid, write_output
    if not os.path.isdir(model.output_dir):
        os.makedirs(model.output_dir, exist_ok=True)
    log = open(os.path.join(model.output_dir, "scythe_out.log"), "w")
    device = None
    if num_tiles > 1:
        device = "cuda"
    run = ModelRun(model, num_tiles=num_tiles, device=device, exchange="auto")
    print("Initializing with %d workers and tiles" % num_tiles, file=log)
    vals = read_physical_grid(model.initial_conditions, model.grid_params, run)
    run.set_initial_conditions(vals)
    num_ts = int(round(model.integration_time / model.ts))
    output_int = int(round(model.output_interval / model.ts))
    print("Integrating %s sec increments for %d timesteps" % (model.ts, num_ts), file=log)
    write_output(run, model, 0.0)
    t0 = time.time()
    for t in range(1, num_ts + 1):
        if verbose:
            print("ts: %s" % (t * model.ts), file=log)
        run.step()
        if output_int > 0 and t % output_int == 0 and t != num_ts:
            write_output(run, model, t * model.ts)
            for g in run.tiles:
                checkCFL(g)
    print("%.6f seconds" % (time.time() - t0), file=log)
    write_output(run, model, model.integration_time)
    for g in run.tiles:
        checkCFL(g)
    print("Model complete!", file=log)
    log.close()
    run.close()
    return True
