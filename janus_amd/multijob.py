"""Helper aggregate-init for many small aggregation jobs of several tasks: the jobs are coalesced
into GPU batches, each prepared by ONE engine call.

Janus makes aggregation jobs of at most `max_aggregation_job_size` reports (500 by default, 100 in
every sample config) and runs many tasks at once, each with its own task id, HPKE keys and verify
key.  `HelperAggregateInit` (helper.py) makes one engine call per job on a context bound to one
verify key; at 100 reports the launch chain, the staging copies and the stream synchronisation of
that call cost more than its arithmetic.  Of all Prio3 preparation only the query randomness reads
the verify key, so the engine takes a key per report (prio3gpu_state_set_verify_keys) and jobs of
different tasks that share one VDAF shape (kind, bits, length, chunk length, XOF) fit one call.

Per job, on the host, steps 1-3 of helper.py run unchanged with the job's own task id and keys:
decode and request-level checks, gather, HPKE open, PlaintextInputShare decode, structural
faults.  Per batch, the surviving jobs' rows are concatenated and prepared on one helper state:
`set_verify_keys` with the tasks' keys and each job's task index repeated over its reports, one
`helper_init` with the combined batch slots, one `update_reports`.  The prep messages and statuses
are then sliced per job and each AggregationJobResp is encoded on its own.  Task k's batch slot s
is aggregate slot k * slots_per_task + s.

The host stage of batch b + 1 runs on a worker thread while the GPU prepares batch b, as in
`HelperAggregateInit.handle_jobs`.  The request-level decode of every job comes first, on the
calling thread: the packing needs every job's size.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import codec as C
from . import hpke
from ._lib import EmptyAggregation, Prio3GpuError
from .helper import _PinnedPool
from .prio3 import AggregateShares, Prio3Gpu


@dataclass
class HelperTask:
    """What the helper holds per task: `task_id` (32 bytes), the VDAF `verify_key` (16 bytes), its
    HPKE keypairs, and how a report time maps to one of the task's batch slots (None: slot 0)."""
    task_id: bytes
    verify_key: bytes
    task_keys: Sequence[hpke.HpkeKeypair]
    global_keys: Sequence[hpke.HpkeKeypair] = ()
    query_type: int = C.TIME_INTERVAL
    batch_slot_of: Optional[Callable[[np.ndarray], np.ndarray]] = None


def pack_jobs(sizes: Sequence[int], max_reports: int) -> List[List[int]]:
    """Job indices per GPU batch.  Jobs stay in order and are never split; a batch holds at most
    `max_reports` reports, except that a single job larger than that forms a batch alone; jobs
    of size 0 (rejected requests) are in no batch."""
    if max_reports < 1:
        raise ValueError("max_reports must be at least 1")
    batches: List[List[int]] = []
    cur: List[int] = []
    total = 0
    for j, n in enumerate(sizes):
        if n < 0:
            raise ValueError(f"job {j} has a negative size")
        if n == 0:
            continue
        if cur and total + n > max_reports:
            batches.append(cur)
            cur, total = [], 0
        cur.append(j)
        total += n
    if cur:
        batches.append(cur)
    return batches


def aggregate_slots(task_index: int, slots_per_task: int, task_slots) -> np.ndarray:
    """Aggregate slots of one job's reports: task_index * slots_per_task + the task's own batch
    slot per report (`task_slots`, what its `batch_slot_of` returned).  A slot that is not below
    `slots_per_task` would land in another task's aggregate: `ValueError`."""
    s = np.asarray(task_slots).astype(np.int64)
    bad = np.flatnonzero((s < 0) | (s >= slots_per_task))
    if bad.size:
        raise ValueError(f"batch_slot_of returned slot {int(s[bad[0]])} for a report of task "
                         f"{task_index}: a task has slots 0..{slots_per_task - 1}")
    return (task_index * slots_per_task + s).astype(np.uint32)


@dataclass
class _OpenedBatch:
    jobs: List[int]            # indices into the caller's job list
    offs: List[int]            # row offset of each job, then the total
    nonces: np.ndarray
    public: np.ndarray
    leader_prep: np.ndarray
    helper_in: np.ndarray
    status: np.ndarray
    slots: np.ndarray
    times: np.ndarray
    key_index: np.ndarray
    buf: int = -1              # pinned staging buffer holding leader_prep (-1: none)


class HelperJobBatcher:
    def __init__(self, vdaf: Prio3Gpu, tasks: Sequence[HelperTask], slots_per_task: int = 1,
                 hpke_threads: int = 0, max_reports: int = 65536):
        """`vdaf` gives the VDAF shape every task shares and the GPU context; its own verify key
        is not used.  `max_reports` bounds a GPU batch (see `pack_jobs`)."""
        if not tasks:
            raise ValueError("no tasks")
        if slots_per_task < 1:
            raise ValueError("slots_per_task must be at least 1")
        for t in tasks:
            if len(t.task_id) != 32 or len(t.verify_key) != 16:
                raise ValueError("a task has a 32-byte id and a 16-byte verify key")
        self.vdaf = vdaf
        self.tasks = list(tasks)
        self.slots_per_task = slots_per_task
        self.hpke_threads = hpke_threads
        self.max_reports = max_reports
        self._keys = np.frombuffer(b"".join(bytes(t.verify_key) for t in self.tasks),
                                   np.uint8).reshape(len(self.tasks), 16).copy()
        self._state = None
        self._cap = 0
        self._pinned = _PinnedPool(vdaf.sizes.prep_share)

    def new_aggregate(self) -> AggregateShares:
        return self.vdaf.new_aggregate(len(self.tasks) * self.slots_per_task)

    # -- host stages -------------------------------------------------------------------------------
    def _decode(self, task_index: int, req_bytes):
        """Step 1's decode and request-level checks.  Raises for the request alone."""
        if not 0 <= task_index < len(self.tasks):
            raise ValueError(f"job names task {task_index} of {len(self.tasks)}")
        req = C.decode_agg_init_req(req_bytes, self.tasks[task_index].query_type)
        C.check_agg_init_req(req)
        if req.n == 0:
            raise EmptyAggregation("aggregation job contains no reports")
        return req

    def _open_batch(self, jobs: List[int], task_of: Sequence[int], reqs) -> _OpenedBatch:
        """Steps 1-3 of every job of one batch, into the batch's combined rows."""
        s = self.vdaf.sizes
        offs = [0]
        for j in jobs:
            offs.append(offs[-1] + reqs[j].n)
        total = offs[-1]
        k, buf = self._pinned.acquire(total)
        try:
            lps = buf[:total] if buf is not None else np.zeros((total, s.prep_share), np.uint8)
            nonces = np.zeros((total, 16), np.uint8)
            public = np.zeros((total, s.public_share), np.uint8)
            helper_in = np.zeros((total, s.helper_input_share), np.uint8)
            status = np.zeros(total, np.uint8)
            slots = np.zeros(total, np.uint32)
            times = np.zeros(total, np.uint64)
            key_index = np.zeros(total, np.uint32)
            for j, lo, hi in zip(jobs, offs[:-1], offs[1:]):
                t, req = self.tasks[task_of[j]], reqs[j]
                nz, pub, _, faults = C.gather_prepare_inits(s, req, lps_out=lps[lo:hi])
                pts, po, st = hpke.open_report_shares(t.task_id, req, list(t.task_keys),
                                                      list(t.global_keys), None, self.hpke_threads)
                hin, st = C.decode_plaintext_input_shares_raw(s, pts, po, 1, st)
                C.apply_faults(st, faults)
                tm = req.times()
                local = np.zeros(req.n, np.uint32) if t.batch_slot_of is None \
                    else t.batch_slot_of(tm)
                nonces[lo:hi], public[lo:hi], helper_in[lo:hi] = nz, pub, hin
                status[lo:hi], times[lo:hi] = st, tm
                slots[lo:hi] = aggregate_slots(task_of[j], self.slots_per_task, local)
                key_index[lo:hi] = task_of[j]
        except BaseException:
            self._pinned.release(k)
            raise
        return _OpenedBatch(list(jobs), offs, nonces, public, lps, helper_in, status, slots, times,
                            key_index, k)

    # -- GPU stage ---------------------------------------------------------------------------------
    def _prepare(self, o: _OpenedBatch, agg: AggregateShares) -> List[Tuple[int, bytes]]:
        """Steps 4-5: one keyed helper_init and one update_reports for the batch, then every
        job's own AggregationJobResp."""
        total = o.offs[-1]
        try:
            if total > self._cap:
                if self._state is not None:
                    self._state.close()
                self._cap = max(total, 2 * self._cap)
                self._state = self.vdaf.new_state(1, self._cap)
            self._state.set_verify_keys(self._keys, o.key_index)
            msgs, st = self.vdaf.helper_init(self._state, o.nonces, o.public, o.helper_in,
                                             o.leader_prep, agg=agg, batch_slots=o.slots,
                                             status=o.status)
        finally:
            self._pinned.release(o.buf)  # the engine call returns after its stream has synchronised
            o.buf = -1
        agg.update_reports(o.nonces, o.times, st, o.slots)
        pm = self.vdaf.sizes.prep_msg
        return [(j, C.encode_agg_job_resp(o.nonces[lo:hi], None if msgs is None else msgs[lo:hi],
                                          pm, st[lo:hi]))
                for j, lo, hi in zip(o.jobs, o.offs[:-1], o.offs[1:])]

    def handle_jobs(self, jobs: Sequence[Tuple[int, bytes]], agg: AggregateShares) -> List[object]:
        """`jobs`: (task index, AggregationJobInitializeReq bytes) in any interleaving.  Entry j of
        the result is job j's AggregationJobResp bytes, or the Prio3GpuError that failed that
        request alone (InvalidMessage: duplicate report IDs or a non-empty aggregation parameter;
        EmptyAggregation), as `HelperAggregateInit.handle_jobs` answers it.  An engine failure
        while a batch is prepared ends the stream (re-raised), after the staging buffer of the
        batch opened ahead is released."""
        if agg.num_slots != len(self.tasks) * self.slots_per_task:
            raise ValueError(f"aggregate has {agg.num_slots} slots; the batcher's tasks need "
                             f"{len(self.tasks) * self.slots_per_task} (new_aggregate)")
        out: List[object] = [None] * len(jobs)
        reqs: List[object] = [None] * len(jobs)
        task_of = [int(t) for t, _ in jobs]
        sizes = [0] * len(jobs)
        for j, (t, req_bytes) in enumerate(jobs):
            try:
                reqs[j] = self._decode(t, req_bytes)
                sizes[j] = reqs[j].n
            except Prio3GpuError as e:  # this request alone is rejected
                out[j] = e
        batches = pack_jobs(sizes, self.max_reports)
        if not batches:
            return out
        with ThreadPoolExecutor(max_workers=1) as pool:
            nxt = pool.submit(self._open_batch, batches[0], task_of, reqs)
            for b in range(len(batches)):
                cur = nxt.result()
                if b + 1 < len(batches):
                    nxt = pool.submit(self._open_batch, batches[b + 1], task_of, reqs)
                try:
                    for j, resp in self._prepare(cur, agg):
                        out[j] = resp
                except BaseException:
                    if b + 1 < len(batches):  # drain the batch opened ahead and free its buffer
                        try:
                            ahead = nxt.result()
                        except BaseException:
                            ahead = None
                        if isinstance(ahead, _OpenedBatch):
                            self._pinned.release(ahead.buf)
                    raise
        return out

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None
        self._pinned.clear()
