"""The staged file pipeline behind `core.files_to_scores` and
`data.preprocess.from_files_to_files`, and where its threads run.  Host code
only: the stages are the callers' callables."""
import collections
import concurrent.futures
import contextlib
import os
import threading

from . import files
from . import runtime

# the library's file pool belongs to the process: the calls that have placed
# it, and where it goes back to when the last of them ends
_LOCK = threading.Lock()
_users, _everywhere = 0, None


@contextlib.contextmanager
def near_gpu(device_index, threads_needed):
    """The threads of `run` and the library's file pool - ours, never the
    caller's - next to GPU `device_index`, whose DMA engine reads what they
    copy into pinned memory, when its node has room for `threads_needed` of
    them (packed onto a few near CPUs, pools sized from the whole CPU budget
    would lose more than the far socket costs).  Yields the `initializer` of
    `run`, or None: placement is a nicety, never a failure.  The pool is
    shared, so its users are counted: the first call to enter places it, one
    that enters meanwhile leaves it there (and still settles its own threads
    near its own GPU), the last one to leave sends it back to every CPU."""
    global _users, _everywhere
    near, placed = files.cpus_near(device_index), False
    if near is not None and len(near) >= threads_needed:
        with _LOCK, contextlib.suppress(runtime.LibraryError, OSError):
            if not _users:
                _everywhere = sorted(os.sched_getaffinity(0))
                files.pool_near(near)
            _users += 1
            placed = True

    def settle():
        with contextlib.suppress(OSError):      # (a cpuset that changed: stay)
            os.sched_setaffinity(0, near)       # (pid 0: this thread only)
    try:
        yield settle if placed else None
    finally:
        if placed:
            with _LOCK:
                _users -= 1
                if not _users:
                    with contextlib.suppress(runtime.LibraryError):
                        files.pool_near(_everywhere)


def run(count, open, submit, write, collect=None, *, openers, ahead,
        unwritten, initializer=None):
    """`count` batches through three stages that run side by side:

        open(position) -> job           on `openers` threads, at most `ahead`
                                        batches in front of the caller's
        submit(position, job) -> item   on the calling thread
        write(position, item)           on the writer thread

    With `collect`, batch i is written a batch later: once batch i + 1 is
    submitted, `collect(i, item)` runs on the calling thread and every element
    it yields is written.  A batch is submitted once at most `unwritten`
    writes are pending.  The first failure of a stage (an interrupt too) is
    kept: what was submitted is still collected and written, every write is
    joined, unopened batches are cancelled, the threads end - then it is
    raised."""
    opener = concurrent.futures.ThreadPoolExecutor(
        openers, thread_name_prefix='emphases-open', initializer=initializer)
    writer = concurrent.futures.ThreadPoolExecutor(
        1, thread_name_prefix='emphases-write', initializer=initializer)
    opening, submitted, writes = (collections.deque() for _ in range(3))
    failures, lag = [], 0 if collect is None else 1

    @contextlib.contextmanager
    def kept():
        try:
            yield
        except BaseException as error:      # noqa: BLE001
            failures.append(error)

    def queue(position, item):
        for element in [item] if collect is None else collect(position, item):
            writes.append(writer.submit(write, position, element))

    with kept():
        opening.extend(opener.submit(open, position)
                       for position in range(min(ahead, count)))
        for position in range(count):
            job = opening.popleft().result()
            while len(writes) > unwritten:  # (errors surface; memory bounded)
                writes.popleft().result()
            if position + ahead < count:
                opening.append(opener.submit(open, position + ahead))
            submitted.append((position, submit(position, job)))
            if len(submitted) > lag:
                queue(*submitted.popleft())
    with kept():
        while submitted:
            queue(*submitted.popleft())
    for pending in writes:
        with kept():
            pending.result()
    opener.shutdown(wait=True, cancel_futures=True)
    writer.shutdown(wait=True)
    if failures:
        raise failures[0]
