"""`emphases_amd.pipeline` without a GPU: the staged loop under fake stages
that record (stage, position, thread) and sleep or raise on request, and the
counted placement of the shared file pool under a fake `files.pool_near`."""
import os
import threading
import time

import pytest

from emphases_amd import files, pipeline, runtime

# (openers, ahead, unwritten, with a collect stage): the file API's shape and
# the feature cache's
SHAPES = [(2, 2, 2, True), (1, 2, 1, False)]
COUNT = 10


class Stages:
    """The stages of `pipeline.run` as recorders: `events` holds (stage,
    position, thread name, 'start' | 'end') in the order things happened."""

    def __init__(self, collect, slow=None, seconds=0.02, fail=None,
                 elements=1):
        self.events, self.elements = [], elements
        self.slow, self.seconds = slow, seconds
        self.fail = fail or {}          # (stage, position) -> exception
        self.collect = self._collect if collect else None

    def _stage(self, stage, position):
        name = threading.current_thread().name
        self.events.append((stage, position, name, 'start'))
        if stage == self.slow:
            time.sleep(self.seconds)
        if (stage, position) in self.fail:
            raise self.fail[stage, position]
        self.events.append((stage, position, name, 'end'))

    def open(self, position):
        self._stage('open', position)
        return 'job', position

    def submit(self, position, job):
        assert job == ('job', position)
        self._stage('submit', position)
        return 'item', position

    def _collect(self, position, item):
        assert item == ('item', position)
        self._stage('collect', position)
        # (several submissions of one batch, as for several sample rates)
        return (('scores', position) for _ in range(self.elements))

    def write(self, position, element):
        assert element in (('item', position), ('scores', position))
        self._stage('write', position)

    def run(self, shape, count=COUNT):
        openers, ahead, unwritten, _ = shape
        pipeline.run(count, self.open, self.submit, self.write, self.collect,
                     openers=openers, ahead=ahead, unwritten=unwritten)

    def index(self, stage, position, edge):
        return [event[:2] + event[3:] for event in self.events].index(
            (stage, position, edge))

    def positions(self, stage, edge='end'):
        return [event[1] for event in self.events
                if event[0] == stage and event[3] == edge]


def _stage_threads():
    return [thread.name for thread in threading.enumerate()
            if thread.name.startswith(('emphases-open', 'emphases-write'))]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('slow', [None, 'open', 'submit', 'write'])
def test_stage_order(shape, slow):
    """open, submit, (collect,) write for every batch; submit and collect on
    the calling thread, the others on threads named for their stage; what
    shares a thread runs in batch order; a batch is collected once the next
    one is submitted."""
    stages = Stages(shape[3], slow, 0.005)
    stages.run(shape)
    chain = ['open', 'submit'] + ['collect'] * shape[3] + ['write']
    for position in range(COUNT):
        marks = [stages.index(stage, position, edge)
                 for stage in chain for edge in ('start', 'end')]
        assert marks == sorted(marks), (position, marks)
        if shape[3] and position + 1 < COUNT:
            assert stages.index('submit', position + 1, 'end') < \
                stages.index('collect', position, 'start')
    caller = threading.current_thread().name
    prefixes = {'open': 'emphases-open', 'write': 'emphases-write',
                'submit': caller, 'collect': caller}
    order = {}
    for stage, position, name, edge in stages.events:
        assert name.startswith(prefixes[stage]), (stage, name)
        if edge == 'start':
            order.setdefault((name, stage), []).append(position)
    for ran in order.values():
        assert ran == sorted(ran), order
    for stage in chain[1:]:
        assert stages.positions(stage) == list(range(COUNT)), stage
    assert sorted(stages.positions('open')) == list(range(COUNT))
    assert len({name for name, stage in order if stage == 'open'}) <= shape[0]
    assert _stage_threads() == []


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('slow', ['write', 'open', 'submit'])
def test_opening_ahead_and_unwritten_bound(shape, slow):
    """Batch p + ahead is not opened before the caller has taken batch p (it
    takes it once batch p is open and batch p - 1 submitted), and no batch is
    submitted while more than `unwritten` writes are pending."""
    _, ahead, unwritten, collect = shape
    stages = Stages(collect, slow)
    stages.run(shape)
    for position in range(COUNT - ahead):
        began = stages.index('open', position + ahead, 'start')
        assert began > stages.index('open', position, 'end'), position
        if position:
            assert began > stages.index('submit', position - 1, 'end'), position
    # a write is queued when its batch is submitted - or, with a collect
    # stage, collected: when the batch after it is
    worst = 0
    for position in range(COUNT):
        before = stages.events[:stages.index('submit', position, 'start')]
        queued = position - 1 if collect else position
        written = sum(1 for event in before
                      if event[0] == 'write' and event[3] == 'end')
        assert queued - written <= unwritten, (position, before)
        worst = max(worst, queued - written)
    if slow == 'write':
        assert worst == unwritten       # (the bound was what held the caller)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('error', [RuntimeError, KeyboardInterrupt])
@pytest.mark.parametrize('stage', ['open', 'submit', 'write'])
def test_failure_keeps_what_was_submitted(shape, error, stage):
    """A stage of batch k fails (an interrupt takes the same way): every batch
    submitted before that is collected and written, none is submitted after
    it, the failure itself is raised, and the stages' threads are gone."""
    k, (_, _, unwritten, collect) = 4, shape
    failure = error(f'{stage} of batch {k}')
    stages = Stages(collect, fail={(stage, k): failure})
    with pytest.raises(error) as caught:
        stages.run(shape)
    assert caught.value is failure
    submitted = stages.positions('submit', 'start')
    if stage == 'write':
        # noticed when the caller next waits for that write
        assert submitted == list(range(len(submitted)))
        assert k < len(submitted) <= k + unwritten + 1 + collect < COUNT
        done = [p for p in submitted if p != k]
    else:
        assert submitted == list(range(k + (stage == 'submit')))
        done = list(range(k))
    assert stages.positions('write') == done
    if collect:
        assert stages.positions('collect') == (
            submitted if stage == 'write' else done)
    assert _stage_threads() == []


def test_first_failure_is_the_one_raised():
    """Batch 3 fails in submit, then the write of batch 2 - queued on the way
    out - fails as well: the first is raised, the others are still written."""
    first, second = ValueError('submit'), OSError('write')
    stages = Stages(True, fail={('submit', 3): first, ('write', 2): second})
    with pytest.raises(ValueError) as caught:
        stages.run(SHAPES[0])
    assert caught.value is first
    assert stages.positions('collect') == [0, 1, 2]
    assert stages.positions('write', 'start') == [0, 1, 2]
    assert stages.positions('write') == [0, 1]
    assert _stage_threads() == []


def test_every_element_of_a_batch_is_written():
    """A batch that yields two submissions: two writes, batch after batch."""
    stages = Stages(True, elements=2)
    stages.run(SHAPES[0], count=4)
    assert stages.positions('write') == [0, 0, 1, 1, 2, 2, 3, 3]


def test_no_batches():
    stages = Stages(True)
    stages.run(SHAPES[0], count=0)
    assert stages.events == [] and _stage_threads() == []


###############################################################################
# Placement
###############################################################################


@pytest.fixture
def pool(monkeypatch):
    """`files.cpus_near` answers with two of the process's own CPUs for GPU 0
    and one of them for GPU 1; the calls of `files.pool_near` are recorded."""
    allowed = sorted(os.sched_getaffinity(0))
    near = {0: allowed[:2], 1: allowed[:1]}
    calls = []
    monkeypatch.setattr(files, 'cpus_near', near.get)
    monkeypatch.setattr(files, 'pool_near', lambda cpus: calls.append(cpus))
    return near, calls, allowed


def _affinity_under(initializer):
    """Where a fresh thread may run after `initializer`."""
    seen = []
    thread = threading.Thread(
        target=lambda: (initializer(), seen.append(os.sched_getaffinity(0))))
    thread.start()
    thread.join()
    return sorted(seen[0])


def test_overlapping_calls_share_one_placement(pool):
    """Two calls overlap on two threads: the pool is placed once, by the
    first, and sent back once, after the second has left too.  The second -
    another GPU, another node - still settles its own threads near its GPU."""
    near, calls, allowed = pool
    events, inside = [], [threading.Event(), threading.Event()]
    settled = {}

    def first():
        with pipeline.near_gpu(0, len(near[0])) as settle:
            settled[0] = _affinity_under(settle)
            inside[0].set()
            inside[1].wait(10)
        events.append(('left', 0, list(calls)))

    def second():
        inside[0].wait(10)
        with pipeline.near_gpu(1, 1) as settle:
            settled[1] = _affinity_under(settle)
            inside[1].set()
            threads[0].join(10)
            events.append(('leaving', 1, list(calls)))
        events.append(('left', 1, list(calls)))

    threads = [threading.Thread(target=first), threading.Thread(target=second)]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join(10)
    assert [event[:2] for event in events] == [
        ('left', 0), ('leaving', 1), ('left', 1)]
    assert events[0][2] == events[1][2] == [near[0]]
    assert calls == [near[0], allowed]
    assert settled == {0: near[0], 1: near[1]}


def test_single_call_places_and_restores(pool):
    """One call: the pool near the GPU inside, everywhere after, the threads
    of `run` on the near CPUs - and the caller's thread where it was."""
    near, calls, allowed = pool
    before = os.sched_getaffinity(0)
    seen = {}

    def stage(name):
        def record(position, *_):
            seen.setdefault(name, set()).add(
                tuple(sorted(os.sched_getaffinity(0))))
        return record

    with pipeline.near_gpu(0, len(near[0])) as settle:
        assert calls == [near[0]]
        assert os.sched_getaffinity(0) == before
        pipeline.run(3, stage('open'), stage('submit'), stage('write'),
                     openers=1, ahead=2, unwritten=1, initializer=settle)
        assert os.sched_getaffinity(0) == before
    assert calls == [near[0], allowed]
    assert os.sched_getaffinity(0) == before
    assert seen == {'open': {tuple(near[0])}, 'write': {tuple(near[0])},
                    'submit': {tuple(sorted(before))}}


def test_placement_is_a_nicety(pool, monkeypatch):
    """A pool that refuses on the way in: no initializer, no error, and the
    refused call is not counted as a user of the pool."""
    near, calls, allowed = pool

    def refuse(cpus):
        raise runtime.LibraryError('emph_files_affinity failed')
    monkeypatch.setattr(files, 'pool_near', refuse)
    before = os.sched_getaffinity(0)
    with pipeline.near_gpu(0, len(near[0])) as settle:
        assert settle is None
        assert os.sched_getaffinity(0) == before
    monkeypatch.setattr(files, 'pool_near', lambda cpus: calls.append(cpus))
    with pipeline.near_gpu(0, len(near[0])) as settle:
        assert settle is not None and calls == [near[0]]
    assert calls == [near[0], allowed]
    # ... and one that refuses on the way out is no error either
    with pipeline.near_gpu(0, len(near[0])):
        monkeypatch.setattr(files, 'pool_near', refuse)
    monkeypatch.setattr(files, 'pool_near', lambda cpus: calls.append(cpus))
    with pipeline.near_gpu(0, len(near[0])):
        pass
    assert calls == [near[0], allowed, near[0], near[0], allowed]


def test_no_node_or_no_room_places_nothing(pool, monkeypatch):
    """`cpus_near` does not know, or the node is too small for the threads:
    nothing is called, nothing is yielded."""
    near, calls, _ = pool
    touched = []
    monkeypatch.setattr(os, 'sched_setaffinity',
                        lambda *args: touched.append(args))
    with pipeline.near_gpu(0, len(near[0]) + 1) as settle:
        assert settle is None
    monkeypatch.setattr(files, 'cpus_near', lambda index: None)
    with pipeline.near_gpu(0, 1) as settle:
        assert settle is None
    assert calls == [] and touched == []
