"""``Communicator``: the framework's public communicator façade.

Same API and byte accounting as the reference ``mpi_wrapper/comm.py:4-199``
(``Get_size/Get_rank/Barrier``, library ``Allreduce/Allgather/Reduce_scatter/
Alltoall/Split(key, color)``, hand-written ``myAllreduce/myAlltoall/
myAlltoall2``, ``total_bytes_transferred``), dispatching on the buffer type:

* NumPy arrays / CPU tensors -> the C++ shared-memory host plane (``mpi.py``);
* CUDA tensors               -> the device plane (``device.py``): hand-written
  CDNA4 kernels over IPC-mapped peer HBM (xGMI), RCCL for the library baseline
  and the P2P ring / recursive-halving-doubling schedules.

Deliberate fixes of reference hazards: the reduction op is
validated on every rank *before* any communication (the reference validates on
root only, after the first Recv, so non-roots hang — comm.py:88-95,104-105).
"""
from __future__ import annotations

import sys
from typing import Optional

import numpy as np

from . import _native
from . import mpi as MPI

_h = _native.host()
_fmy_allreduce, _fmy_alltoall = _h.fmy_allreduce, _h.fmy_alltoall
_HOST_ALGOS = {"reduce_bcast": 0, "ring": 1, "rhd": 2}

_SUPPORTED_MY_OPS = ("SUM", "PROD", "MIN", "MAX")


def _is_device(x) -> bool:
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _nbytes_items(x):
    """(itemsize, size) of a NumPy array or torch tensor, like ndarray.itemsize/.size."""
    if _is_device(x) or (sys.modules.get("torch") is not None and isinstance(x, sys.modules["torch"].Tensor)):
        return x.element_size(), x.numel()
    return x.itemsize, x.size


def _np_op(op):
    name = getattr(op, "name", str(op)).upper()
    if name == "SUM":
        return np.add
    if name == "MIN":
        return np.minimum
    if name == "MAX":
        return np.maximum
    if name == "PROD":
        return np.multiply
    raise NotImplementedError("Only MPI.SUM, MPI.MIN, MPI.MAX and MPI.PROD are supported.")


# fast-path lookup of the hand-written ops by the library's Op objects (hashable by code)
_MY_OP_CODE = {getattr(MPI, n): i for i, n in enumerate(_SUPPORTED_MY_OPS) if hasattr(MPI, n)}


def _op_code(op) -> int:
    return _SUPPORTED_MY_OPS.index(getattr(op, "name", str(op)).upper())


def _validate_op(op) -> None:
    name = getattr(op, "name", str(op)).upper()
    if name not in _SUPPORTED_MY_OPS:
        raise NotImplementedError("Only MPI.SUM, MPI.MIN, MPI.MAX and MPI.PROD are supported.")


class DeviceRequest(MPI.Request):
    """MPI-style handle of a device collective started on the communication
    stream (``DeviceGroup.start``).  CUDA-aware-MPI semantics: ``Wait()`` orders
    the caller's current stream after the collective (no host sync), ``Test()``
    polls completion, ``synchronize()`` blocks the host and raises on a device
    timeout.  ``MPI.Request.Waitall`` accepts it mixed with host requests."""

    __slots__ = ()

    def __init__(self, comm, work) -> None:
        super().__init__(comm, work, None)
        self._done = False

    def _finish(self, status=None):
        if not self._done:
            self._result = self._native.wait()
            self._done = True
        return self._result

    def Test(self, status=None) -> bool:
        if self._done:
            return True
        if self._native.is_completed():
            self._finish(status)
            return True
        return False

    def synchronize(self):
        out = self._native.synchronize()
        self._done = True
        return out


class Communicator(object):
    """Reference-compatible communicator with a GPU fast path."""

    def __init__(self, comm=None, device=None):
        self.comm = comm if comm is not None else MPI.COMM_WORLD
        self.total_bytes_transferred = 0
        self._device = device
        self._dev = None
        self._rs = None  # (rank, size): fixed for the communicator's lifetime
        # the hand-written schedules' fast path needs the native host communicator
        self._native_host = isinstance(self.comm, MPI.Comm)

    # ------------------------------------------------------------- identity
    def Get_size(self):
        return self.comm.Get_size()

    def Get_rank(self):
        return self.comm.Get_rank()

    @property
    def rank(self) -> int:
        return self.comm.Get_rank()

    @property
    def size(self) -> int:
        return self.comm.Get_size()

    def Barrier(self):
        if self._dev is not None:
            self._dev.torch.cuda.synchronize(self._dev.device)
        return self.comm.Barrier()

    # --------------------------------------------------------- device plane
    @property
    def dev(self):
        """The device plane of this communicator (created collectively on first use)."""
        if self._dev is None:
            from .device import DeviceGroup

            self._dev = DeviceGroup(self.comm, self._device)
        return self._dev

    def empty(self, shape, dtype=None):
        """Symmetric device allocation (collective): zero-copy collectives."""
        return self.dev.empty(shape, dtype)

    # ---------------------------------------------- library collectives
    def Allreduce(self, src_array, dest_array, op=MPI.SUM, algo: str = "auto"):
        isz, n = _nbytes_items(src_array)
        _, dn = _nbytes_items(dest_array)
        assert n == dn
        src_array_byte = isz * n
        self.total_bytes_transferred += src_array_byte * 2 * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            self.dev.allreduce(src_array, dest_array, op, algo)
        else:
            self.comm.Allreduce(src_array, dest_array, op)

    def Allgather(self, src_array, dest_array, algo: str = "direct"):
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        self.total_bytes_transferred += sisz * sn * (self.comm.Get_size() - 1)
        self.total_bytes_transferred += disz * dn * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            self.dev.allgather(src_array, dest_array, algo)
        else:
            self.comm.Allgather(src_array, dest_array)

    def Reduce_scatter(self, src_array, dest_array, op=MPI.SUM, algo: str = "direct"):
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        self.total_bytes_transferred += sisz * sn * (self.comm.Get_size() - 1)
        self.total_bytes_transferred += disz * dn * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            self.dev.reduce_scatter(src_array, dest_array, op, algo)
        else:
            self.comm.Reduce_scatter_block(src_array, dest_array, op)

    def Split(self, key, color):
        """Note the reference's positional order ``(key, color)`` (comm.py:38).

        The child starts with a fresh byte counter.  When this communicator
        already has an RCCL communicator, the child's is derived with
        ncclCommSplit (collective over this communicator) instead of being
        bootstrapped from scratch."""
        child = self.comm.Split(key=key, color=color)
        out = None if child is MPI.COMM_NULL else __class__(child, self._device)
        if self._dev is not None and self._dev._rccl:
            cdev = out.dev if out is not None else None
            self._dev.split_rccl_into(cdev, -1 if out is None else int(color), int(key))
        return out

    def Alltoall(self, src_array, dest_array, algo: str = "direct"):
        nprocs = self.comm.Get_size()
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        assert sn % nprocs == 0, "src_array size must be divisible by the number of processes"
        assert dn % nprocs == 0, "dest_array size must be divisible by the number of processes"
        send_seg_bytes = sisz * (sn // nprocs)
        recv_seg_bytes = disz * (dn // nprocs)
        self.total_bytes_transferred += send_seg_bytes * (nprocs - 1)
        self.total_bytes_transferred += recv_seg_bytes * (nprocs - 1)
        if _is_device(src_array):
            self.dev.alltoall(src_array, dest_array, algo)
        else:
            self.comm.Alltoall(src_array, dest_array)

    def Alltoallv(self, src_array, send_counts, dest_array, recv_counts, algo: str = "auto"):
        """All-to-all with per-rank element counts, packed in rank order on both sides
        (MPI Alltoallv without explicit displacements; the MoE dispatch shape).
        Accounting: the bytes this rank sends to and receives from the other ranks."""
        rank, p = self.comm.Get_rank(), self.comm.Get_size()
        isz, _ = _nbytes_items(src_array)
        self.total_bytes_transferred += isz * (sum(int(c) for j, c in enumerate(send_counts) if j != rank) +
                                               sum(int(c) for i, c in enumerate(recv_counts) if i != rank))
        if _is_device(src_array):
            self.dev.alltoallv(src_array, send_counts, dest_array, recv_counts)
        else:
            self.comm.Alltoallv([src_array, list(send_counts)], [dest_array, list(recv_counts)])

    def moe_dispatch(self, x, topk_idx, num_experts: int, recv_x, max_blocks=None, *, expert_capacity=None):
        """Routed MoE token dispatch of CUDA tensors (``DeviceGroup.moe_dispatch``): ``x``
        [T, D] and the router's ``topk_idx`` [T, K] go in, ``recv_x`` (from ``comm.empty``)
        receives the rows of this rank's experts grouped by expert.  Returns the handle
        ``moe_combine`` takes.  ``expert_capacity`` (the same on every rank) keeps at most
        that many rows per expert and drops the rest without an error
        (``handle.num_dropped``).  ``total_bytes_transferred`` is not advanced: the counts
        never reach the host."""
        if not _is_device(x):
            raise TypeError("moe_dispatch runs on the device plane: x must be a CUDA tensor")
        return self.dev.moe_dispatch(x, topk_idx, num_experts, recv_x, max_blocks, expert_capacity=expert_capacity)

    def moe_combine(self, y, handle, weights=None, out=None, max_blocks=None):
        """Weighted combine of the expert outputs ``y`` back onto the source tokens
        (``DeviceGroup.moe_combine``).  ``total_bytes_transferred`` is not advanced: the
        counts never reach the host."""
        if not _is_device(y):
            raise TypeError("moe_combine runs on the device plane: y must be a CUDA tensor")
        return self.dev.moe_combine(y, handle, weights, out, max_blocks)

    def moe_combine_backward(self, dout, handle, weights=None, y=None, dy=None, max_blocks=None):
        """Backward of ``moe_combine`` (``DeviceGroup.moe_combine_backward``): ``dout`` goes
        in, ``(dy, dweights)`` come out -- ``dy`` in the owners' symmetric buffers,
        ``dweights`` only when the forward's ``y`` is given.  ``total_bytes_transferred``
        is not advanced: the counts never reach the host."""
        if not _is_device(dout):
            raise TypeError("moe_combine_backward runs on the device plane: dout must be a CUDA tensor")
        return self.dev.moe_combine_backward(dout, handle, weights, y, dy, max_blocks)

    def Bcast(self, buf, root: int = 0):
        isz, n = _nbytes_items(buf)
        if self.comm.Get_rank() == root:
            self.total_bytes_transferred += isz * n * (self.comm.Get_size() - 1)
        else:
            self.total_bytes_transferred += isz * n
        if _is_device(buf):
            self.dev.bcast(buf, root)
        else:
            self.comm.Bcast(buf, root)

    # ------------------------------------------- non-blocking collectives
    # MPI-3 style: each returns a Request (``Wait`` / ``Test`` / ``Request.Waitall``).
    # NumPy buffers run as round schedules on the host plane (csrc/host/nbcoll.cpp),
    # advanced by every progress call; CUDA tensors run on the device plane's
    # communication stream beside the caller's compute (``DeviceGroup.start``).
    # Byte accounting is that of the blocking call.
    def Iallreduce(self, src_array, dest_array, op=MPI.SUM, algo: str = "auto"):
        isz, n = _nbytes_items(src_array)
        self.total_bytes_transferred += isz * n * 2 * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            return DeviceRequest(self.comm, self.dev.start("allreduce", src_array, dest_array, op, algo))
        return self.comm.Iallreduce(src_array, dest_array, op)

    def Iallgather(self, src_array, dest_array, algo: str = "direct"):
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        self.total_bytes_transferred += (sisz * sn + disz * dn) * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            return DeviceRequest(self.comm, self.dev.start("allgather", src_array, dest_array, algo))
        return self.comm.Iallgather(src_array, dest_array)

    def Ireduce_scatter(self, src_array, dest_array, op=MPI.SUM, algo: str = "direct"):
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        self.total_bytes_transferred += (sisz * sn + disz * dn) * (self.comm.Get_size() - 1)
        if _is_device(src_array):
            return DeviceRequest(self.comm, self.dev.start("reduce_scatter", src_array, dest_array, op, algo))
        return self.comm.Ireduce_scatter_block(src_array, dest_array, op)

    def Ialltoall(self, src_array, dest_array, algo: str = "direct"):
        nprocs = self.comm.Get_size()
        sisz, sn = _nbytes_items(src_array)
        disz, dn = _nbytes_items(dest_array)
        assert sn % nprocs == 0 and dn % nprocs == 0, "buffer sizes must be divisible by the number of processes"
        self.total_bytes_transferred += (sisz * (sn // nprocs) + disz * (dn // nprocs)) * (nprocs - 1)
        if _is_device(src_array):
            return DeviceRequest(self.comm, self.dev.start("alltoall", src_array, dest_array, algo))
        return self.comm.Ialltoall(src_array, dest_array)

    def Ibcast(self, buf, root: int = 0):
        isz, n = _nbytes_items(buf)
        self.total_bytes_transferred += isz * n * ((self.comm.Get_size() - 1) if self.comm.Get_rank() == root else 1)
        if _is_device(buf):
            return DeviceRequest(self.comm, self.dev.start("bcast", buf, root))
        return self.comm.Ibcast(buf, root)

    def Ibarrier(self):
        return self.comm.Ibarrier()

    # object collectives (the reference calls these on raw mpi4py comms:
    # model/func_impl.py:89,107,184) -- provided here too so a Communicator
    # can be passed wherever a raw comm is expected.
    def allgather(self, obj):
        return self.comm.allgather(obj)

    def alltoall(self, objs):
        return self.comm.alltoall(objs)

    def bcast(self, obj, root: int = 0):
        return self.comm.bcast(obj, root)

    def allreduce(self, obj, op=MPI.SUM):
        return self.comm.allreduce(obj, op)

    def barrier(self):
        return self.Barrier()

    # ------------------------------------------------ hand-written collectives
    def myAllreduce(self, src_array, dest_array, op=MPI.SUM, algo: str = "reduce_bcast"):
        """Hand-written all-reduce.

        ``algo="reduce_bcast"`` is the reference algorithm (comm.py:63-107):
        rank 0 receives every rank's buffer in rank order, reduces, then sends
        the result back; accounting root ``2S(p-1)``, others ``2S``.  Also
        ``"ring"`` and ``"rhd"`` (recursive halving/doubling) built from P2P
        messages, and on device tensors every device algorithm
        (``"oneshot" | "twoshot" | "reduce_bcast" | "ring" | "rhd" | "auto"``).
        """
        # fast path: NumPy arrays on the native host plane -- a handful of dict / type checks
        # in front of the native schedule (the general path's checks cost ~1.5 us per call,
        # on the order of one of the schedule's shared-memory messages)
        p = self.comm._p if self._native_host else None
        if p is not None and type(src_array) is np.ndarray and type(dest_array) is np.ndarray:
            code, a = _MY_OP_CODE.get(op), _HOST_ALGOS.get(algo)
            if code is not None and a is not None and \
                    _fmy_allreduce(p, src_array, dest_array, code, a) is not NotImplemented:
                self._account_allreduce(src_array.nbytes, algo)
                return
        _validate_op(op)  # on every rank, before communicating
        if not _is_device(dest_array) and not dest_array.flags.c_contiguous:
            # every schedule receives into / reduces in a flat view of dest
            tmp = np.empty(dest_array.shape, dest_array.dtype)
            self.myAllreduce(src_array, tmp, op, algo)
            dest_array[...] = tmp
            return
        rank = self.comm.Get_rank()
        size = self.comm.Get_size()
        isz, n = _nbytes_items(src_array)
        bytes_transferred = isz * n
        if _is_device(src_array):
            self.dev.allreduce(src_array, dest_array, op, algo)
        elif algo in _HOST_ALGOS and isinstance(self.comm, MPI.Comm) and \
                _fmy_allreduce(self.comm._p, src_array, dest_array, _op_code(op), _HOST_ALGOS[algo]) is not NotImplemented:
            pass  # the same message schedule, run natively (csrc/host/p2p_algos.cpp)
        elif algo == "reduce_bcast":
            self._host_reduce_bcast(src_array, dest_array, op)
        elif algo == "ring":
            self._host_ring(src_array, dest_array, op)
        elif algo == "rhd":
            self._host_rhd(src_array, dest_array, op)
        else:
            raise ValueError(f"unknown myAllreduce algorithm {algo!r}")
        self._account_allreduce(bytes_transferred, algo)

    def _account_allreduce(self, bytes_transferred: int, algo: str) -> None:
        rank, size = self._rank_size()
        if algo == "reduce_bcast":
            if rank == 0:
                self.total_bytes_transferred += 2 * bytes_transferred * (size - 1)
            else:
                self.total_bytes_transferred += 2 * bytes_transferred
        else:
            # ring / rhd / direct: every rank sends and receives 2(p-1)/p of the buffer
            self.total_bytes_transferred += int(2 * 2 * bytes_transferred * (size - 1) / size)

    def _rank_size(self):
        rs = self._rs
        if rs is None:
            rs = self._rs = (self.comm.Get_rank(), self.comm.Get_size())
        return rs

    def _host_reduce_bcast(self, src, dest, op) -> None:
        rank, size = self.comm.Get_rank(), self.comm.Get_size()
        f = _np_op(op)
        if rank == 0:
            np.copyto(dest, src)
            temp = np.empty_like(src)
            for i in range(1, size):
                self.comm.Recv(temp, source=i)
                f(dest, temp, out=dest)
            for i in range(1, size):
                self.comm.Send(dest, dest=i)
        else:
            self.comm.Send(src, dest=0)
            self.comm.Recv(dest, source=0)

    def _host_ring(self, src, dest, op) -> None:
        """Ring reduce-scatter + all-gather over Sendrecv (chunk c owned by rank c+1)."""
        rank, p = self.comm.Get_rank(), self.comm.Get_size()
        f = _np_op(op)
        np.copyto(dest, src)
        if p == 1:
            return
        flat = dest.reshape(-1)
        bounds = [flat.size * i // p for i in range(p + 1)]
        chunk = lambda c: flat[bounds[c % p]:bounds[c % p + 1]]
        right, left = (rank + 1) % p, (rank - 1) % p
        tmp = np.empty(max(bounds[i + 1] - bounds[i] for i in range(p)), dtype=flat.dtype)
        for step in range(p - 1):
            s, r = chunk(rank - step), chunk(rank - step - 1)
            t = tmp[:r.size]
            self.comm.Sendrecv(np.ascontiguousarray(s), dest=right, sendtag=step, recvbuf=t, source=left, recvtag=step)
            f(r, t, out=r)
        for step in range(p - 1):
            s, r = chunk(rank + 1 - step), chunk(rank - step)
            t = tmp[:r.size]
            self.comm.Sendrecv(np.ascontiguousarray(s), dest=right, sendtag=100 + step, recvbuf=t, source=left,
                               recvtag=100 + step)
            r[...] = t

    def _host_rhd(self, src, dest, op) -> None:
        """Recursive halving (reduce-scatter) + doubling (all-gather); power-of-two sizes,
        other sizes fall back to the ring."""
        rank, p = self.comm.Get_rank(), self.comm.Get_size()
        if p & (p - 1):
            return self._host_ring(src, dest, op)
        f = _np_op(op)
        np.copyto(dest, src)
        flat = dest.reshape(-1)
        lo, hi = 0, flat.size
        hist = []
        mask = p // 2
        while mask >= 1:
            partner = rank ^ mask
            mid = lo + (hi - lo) // 2
            keep, send = ((mid, hi), (lo, mid)) if rank & mask else ((lo, mid), (mid, hi))
            t = np.empty(keep[1] - keep[0], dtype=flat.dtype)
            self.comm.Sendrecv(np.ascontiguousarray(flat[send[0]:send[1]]), dest=partner, sendtag=mask,
                               recvbuf=t, source=partner, recvtag=mask)
            f(flat[keep[0]:keep[1]], t, out=flat[keep[0]:keep[1]])
            hist.append((lo, hi))
            lo, hi = keep
            mask //= 2
        mask = 1
        while mask <= p // 2:
            partner = rank ^ mask
            plo, phi = hist.pop()
            olo, ohi = (hi, phi) if lo == plo else (plo, lo)
            t = np.empty(ohi - olo, dtype=flat.dtype)
            self.comm.Sendrecv(np.ascontiguousarray(flat[lo:hi]), dest=partner, sendtag=1000 + mask,
                               recvbuf=t, source=partner, recvtag=1000 + mask)
            flat[olo:ohi] = t
            lo, hi = plo, phi
            mask *= 2

    def myAlltoall(self, src_array, dest_array, algo: str = "direct"):
        """Non-blocking all-to-all (reference comm.py:110-159): every Irecv is posted
        before any Isend, then Waitall.  (The reference docstring says Sendrecv;
        it is Irecv/Isend.)  On device tensors: direct peer-read kernel, ``"push"``
        (peer writes), ``"pairwise"`` (hand-written pairwise rounds),
        ``"pairwise_rccl"`` (RCCL P2P rounds) or ``"rccl"``."""
        p = self.comm._p if self._native_host else None
        if p is not None and type(src_array) is np.ndarray and type(dest_array) is np.ndarray and \
                _fmy_alltoall(p, src_array, dest_array, False) is not NotImplemented:
            rank, size = self._rank_size()
            self.total_bytes_transferred += 2 * src_array.itemsize * (src_array.size // size) * (size - 1)
            return
        rank = self.comm.Get_rank()
        size = self.comm.Get_size()
        isz, n = _nbytes_items(src_array)
        segment_size = n // size
        if _is_device(src_array):
            self.dev.alltoall(src_array, dest_array, algo)
        elif isinstance(self.comm, MPI.Comm) and \
                _fmy_alltoall(self.comm._p, src_array, dest_array, False) is not NotImplemented:
            pass  # Irecv-all / Isend-all / Waitall, run natively (csrc/host/p2p_algos.cpp)
        else:  # Python schedule: non-contiguous buffers, or an mpi4py communicator
            src = src_array.reshape(-1)
            dst = dest_array.reshape(-1) if dest_array.flags.c_contiguous else np.empty(n, dest_array.dtype)
            lo = rank * segment_size
            dst[lo:lo + segment_size] = src[lo:lo + segment_size]
            requests = []
            recv_buffers = {}
            for i in range(size):
                if i != rank:
                    recv_buffers[i] = np.empty(segment_size, dtype=src.dtype)
                    requests.append(self.comm.Irecv(recv_buffers[i], source=i))
            for i in range(size):
                if i != rank:
                    requests.append(self.comm.Isend(src[i * segment_size:(i + 1) * segment_size], dest=i))
            MPI.Request.Waitall(requests)
            for i in range(size):
                if i != rank:
                    dst[i * segment_size:(i + 1) * segment_size] = recv_buffers[i]
            if not dest_array.flags.c_contiguous:
                dest_array[...] = dst.reshape(dest_array.shape)
        bytes_transferred = isz * segment_size
        self.total_bytes_transferred += 2 * bytes_transferred * (size - 1)

    def myAlltoall2(self, src_array, dest_array, algo: str = "pairwise"):
        """Pairwise blocking all-to-all (reference comm.py:162-199): for i in rank
        order, Sendrecv with rank i (deadlock-free: the pair (a, b) is handled at
        step b on rank a and step a on rank b).  On device tensors the hand-written
        pairwise kernel (round k: push to rank + k, wait for rank - k; one peer per
        round over the flag protocol), or ``algo="pairwise_rccl"`` / ``"rccl"``."""
        rank = self.comm.Get_rank()
        size = self.comm.Get_size()
        isz, n = _nbytes_items(src_array)
        chunk_size = n // size
        if _is_device(src_array):
            self.dev.alltoall(src_array, dest_array, algo)
        elif isinstance(self.comm, MPI.Comm) and \
                _fmy_alltoall(self.comm._p, src_array, dest_array, True) is not NotImplemented:
            pass  # pairwise Sendrecv rounds, run natively (csrc/host/p2p_algos.cpp)
        else:  # Python schedule: non-contiguous buffers, or an mpi4py communicator
            src = src_array.reshape(-1)
            dst = dest_array.reshape(-1) if dest_array.flags.c_contiguous else np.empty(n, dest_array.dtype)
            recv_buffer = np.empty(chunk_size, dtype=dst.dtype)
            for i in range(size):
                start, end = i * chunk_size, (i + 1) * chunk_size
                if i == rank:
                    np.copyto(dst[start:end], src[start:end])
                else:
                    self.comm.Sendrecv(src[start:end], dest=i, sendtag=rank, recvbuf=recv_buffer, source=i,
                                       recvtag=i)
                    np.copyto(dst[start:end], recv_buffer)
            if not dest_array.flags.c_contiguous:
                dest_array[...] = dst.reshape(dest_array.shape)
        self.total_bytes_transferred += 2 * isz * chunk_size * (size - 1)
