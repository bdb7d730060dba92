"""Cross-request batching: concurrent requests share one pipeline run, each with its own options, noise and output format.

A run of the pipeline costs about the same for one utterance as for a few dozen (the latency-bound part), so N clients whose
sentences share a run get close to N times the audio of N runs in a row.  Two things make a shared run safe:
  - options per row (sbv2_pipeline_run_opts): a request's sdp_ratio / length_scale / noise scales, and its noise key (seed, sentence number
    WITHIN the request), travel with its rows, so its durations and noise are those of the request run alone;
  - an assist text per request (options.assist): it travels on the request's rows as well (assist_ids / assist_weight); the run holds every
    distinct assist sequence once (model._Batch.set_assist), each row blends the mean of its own, and a sequence's mean depends on nothing but
    that sequence's columns;
  - a fetch per request (sbv2_pipeline_fetch_request, orchestrator.finish_request): each request's rows are joined, resampled, gain-staged and
    encoded as its own signal, from the run's PCM, which is only read.

One worker thread owns the pipeline.  It closes a run by the WINDOW RULE: it takes the first waiting request, then further ones in arrival
order until the next would exceed max_utts rows or max_symbols text symbols (sum of T_text), or max_wait_ms have passed since the first was
taken; a request that alone exceeds a limit runs alone.  The three limits are policy knobs whose defaults are the bench workload's (32
utterances of 257 symbols), not tuned values.  Requests are served in arrival order; an error touches its own request only.
"""
import collections
import math
import os
import threading
import time
from concurrent.futures import Future

from . import model, orchestrator


class _Request:
    def __init__(self, args, future, marks=False):
        self.args, self.future, self.plan, self.marks = args, future, None, bool(marks)
        self.n_utts = self.n_symbols = 0


class RequestBatcher:
    def __init__(self, pipe, max_utts=32, max_symbols=8192, max_wait_ms=2.0, depth=None, clock=time.monotonic, start=True):
        """pipe: the model.Pipeline this batcher owns from now on (nothing else may run or fetch on it).  depth: the pipeline's execution contexts
        (SBV2_PIPELINE_DEPTH, default 2): a run's results live until the run `depth` later is launched, so every fetch of a run happens
        before that.  clock: seconds, monotonic (injected by tests).  start=False: the worker starts with start(), after requests were queued."""
        if depth is None:
            depth = max(1, min(8, int(os.environ.get("SBV2_PIPELINE_DEPTH", "2") or 2)))
        self.pipe, self.max_utts, self.max_symbols, self.max_wait = pipe, int(max_utts), int(max_symbols), max_wait_ms / 1000.0
        self.depth, self._clock = int(depth), clock
        self._cond = threading.Condition()
        self._queue = collections.deque()
        self._closing = False
        self._paused, self._idle, self._dead = 0, False, False   # pause(): the worker launches nothing and has answered everything once _idle
        self._inflight = collections.deque()   # launched runs whose requests are not answered yet, oldest first: (batch, [(request, r0, r1)])
        self._thread = threading.Thread(target=self._work, name="sbv2-batcher", daemon=True)
        self._started = False
        if start:
            self.start()

    def start(self):
        if not self._started:
            self._started = True
            self._thread.start()

    def submit(self, sentences, style_vectors, style_id=0, speaker_id=0, options=None, noise_seed=None, marks=False) -> Future:
        """orchestrator.easy_synthesize's request, answered through a Future of its bytes.  marks=True: orchestrator.easy_synthesize_marks'
        request, answered with (bytes, marks): the marks come from the request's own rows of the shared run (its own fetch, its own timeline)
        and equal those of the request run alone."""
        fut = Future()
        req = _Request((list(sentences), style_vectors, style_id, speaker_id, options, noise_seed), fut, marks)
        with self._cond:
            if self._closing:
                raise model.Sbv2Error("the batcher is closed")
            self._queue.append(req)
            self._cond.notify_all()
        return fut

    def close(self):
        """Drains: every request submitted so far is answered (or fails with its own error), then the worker ends.  The pipeline stays open."""
        with self._cond:
            self._closing = True
            self._cond.notify_all()
        if self._started:
            self._thread.join()
        with self._cond:   # never started: nothing will answer these
            while self._queue:
                self._queue.popleft().future.cancel()

    # ---- the worker ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(options):
        """What sbv2_pipeline_run_opts refuses per row, refused per request before its rows join a run."""
        if not (math.isfinite(options.length_scale) and options.length_scale > 0):
            raise model.Sbv2Error(f"length_scale must be finite and > 0: {options.length_scale}")
        if not 0.0 <= options.sdp_ratio <= 1.0:
            raise model.Sbv2Error(f"sdp_ratio must be in [0, 1]: {options.sdp_ratio}")

    def _plan(self, req):
        """The request's plan and its rows, options and noise key on every row; False (future failed) when the request itself is bad."""
        if not req.future.set_running_or_notify_cancel():
            return False
        try:
            sentences, style_vectors, style_id, speaker_id, options, seed = req.args
            plan = orchestrator.RequestPlan(sentences, style_vectors, style_id, speaker_id, options)
            self._check(plan.options)
            orchestrator.require_formant(self.pipe, plan.options)
            orchestrator.require_assist(self.pipe, plan.options)   # (its rows carry the pair: equal assist ids of a run share one sequence)
            if req.marks:
                orchestrator.envelope_hop(plan.options, plan.fmt.sample_rate)
                orchestrator.pitch_options(plan.options, plan.fmt.sample_rate)
            else:
                orchestrator.refuse_pitch(plan.options, "a request without marks (/synthesize)")
            seed = model.fresh_noise_seed() if seed is None else seed
            for j, u in enumerate(plan.utts):   # noise_index restarts per request: the keys of the request run alone
                u.update(sdp_ratio=plan.options.sdp_ratio, length_scale=plan.options.length_scale, noise_scale=orchestrator.NOISE_SCALE,
                         noise_scale_w=orchestrator.NOISE_SCALE_W, noise_seed=seed, noise_index=j)
            req.plan, req.n_utts, req.n_symbols = plan, len(plan.utts), sum(len(u["phones"]) for u in plan.utts)
            return True
        except Exception as e:
            req.future.set_exception(e)
            return False

    def _take_run(self):
        """The requests of the next run by the window rule; [] when nothing can be assembled now (closing, paused, or runs in flight to answer
        first).  While a run is open and nothing waits, the runs in flight are answered before the worker sleeps towards the deadline."""
        run, utts, symbols, deadline = [], 0, 0, None
        while True:
            with self._cond:
                while True:
                    if self._paused and not self._closing:
                        return run   # launch what is open; the worker then answers everything and idles (_work)
                    if self._queue:
                        break
                    if self._closing or run and self._clock() >= deadline:
                        return run
                    if self._inflight:
                        if not run:
                            return run   # nothing to assemble: answer what is in flight first (the caller comes back)
                        break            # an open run and time to spare: answer them below, outside the lock
                    self._cond.wait(None if not run else max(deadline - self._clock(), 0.0))
                req = self._queue[0] if self._queue else None
                if req is not None and run and self._clock() >= deadline:
                    return run
            if req is None:
                self._trim(0)
                continue
            if req.plan is None and not self._plan(req):   # (outside the lock: submit never waits for a plan; only this thread pops)
                with self._cond:
                    self._queue.popleft()
                continue
            if run and (utts + req.n_utts > self.max_utts or symbols + req.n_symbols > self.max_symbols):
                return run   # (it stays first in the queue: arrival order)
            with self._cond:
                self._queue.popleft()
            if not run:
                deadline = self._clock() + self.max_wait
            run.append(req)
            utts, symbols = utts + req.n_utts, symbols + req.n_symbols
            if utts >= self.max_utts or symbols >= self.max_symbols:
                return run

    def _launch(self, run):
        try:
            b = self.pipe.prepare([u for r in run for u in r.plan.utts])
            self.pipe.run(b)
        except Exception as e:
            self._trim(0)   # a run that failed after it began has used up an execution context: answer what is in flight while its tickets hold
            if len(run) == 1:
                run[0].future.set_exception(e)
                return
            for r in run:   # one of them is refused by the library: each on its own, so that the error stays with its request
                self._launch([r])
                self._trim(self.depth - 1)
            return
        rows, r0 = [], 0
        for r in run:
            rows.append((r, r0, r0 + r.n_utts))
            r0 += r.n_utts
        self._inflight.append((b, rows))

    def _trim(self, keep):
        """Answers the oldest runs in flight until `keep` are left: a run is fetched before the run `depth` launches after it reuses its context."""
        while len(self._inflight) > keep:
            b, rows = self._inflight[0]   # (it leaves the list once answered: a failing worker still finds it, _work)
            pcm = None
            for req, r0, r1 in rows:
                if req.future.done():
                    continue
                try:
                    if req.marks:   # (its own fetch at every format: the levels are taken of its delivered signal)
                        got = []
                        audio = orchestrator.finish_request(self.pipe, b, r0, r1, req.plan, marks=got)
                        req.future.set_result((audio, got[0]))
                        continue
                    if (pcm is None and req.plan.gain is None and req.plan.fmt.is_default and orchestrator.voice_options(req.plan.options) is None
                            and getattr(req.plan, "token_pitch", None) is None and orchestrator.formant_options(req.plan.options) is None):
                        pcm = self.pipe.fetch(b)   # the plain f32 requests of a run share one fetch
                    req.future.set_result(orchestrator.finish_request(self.pipe, b, r0, r1, req.plan, pcm=pcm))
                except Exception as e:
                    req.future.set_exception(e)
            self._inflight.popleft()

    def pause(self):
        """Returns once the worker has answered every run it launched and launches nothing more until resume(): what else uses the pipeline's
        handles meanwhile (a stream of the same model runs on execution context 0 itself) finds them idle.  Requests keep queueing.  Counted:
        pause() twice needs resume() twice."""
        with self._cond:
            self._paused += 1
            self._cond.notify_all()
            while self._started and not self._idle and not self._dead:
                self._cond.wait()

    def resume(self):
        with self._cond:
            self._paused = max(self._paused - 1, 0)
            self._cond.notify_all()

    def _work(self):
        run = []
        try:
            while True:
                run = self._take_run()
                if run:
                    self._trim(self.depth - 1)   # (a fallback in _launch may have left more behind than one launch allows)
                    self._launch(run)
                    run = []
                    self._trim(self.depth - 1)
                    continue
                self._trim(0)
                with self._cond:
                    if self._closing and not self._queue:
                        return
                    while self._paused and not self._closing:   # nothing in flight, nothing launched: the pipeline is the pauser's
                        self._idle = True
                        self._cond.notify_all()
                        self._cond.wait()
                    self._idle = False
        except BaseException as e:   # a bug here must not leave a client waiting for ever
            with self._cond:
                self._closing = True
                pending = [r for r in run] + [r for _, rows in self._inflight for r, _, _ in rows] + list(self._queue)
                self._inflight.clear()
                self._queue.clear()
            for r in pending:
                if not r.future.done():
                    if r.plan is None and not r.future.set_running_or_notify_cancel():
                        continue
                    r.future.set_exception(model.Sbv2Error(f"the batcher's worker failed: {e!r}"))
        finally:
            with self._cond:
                self._dead = True
                self._cond.notify_all()
