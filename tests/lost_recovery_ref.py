"""lost_recovery: restated for the tests: the options, the state machine (mola_hip::LostRecovery) as a plain Python fold, and the CPU
oracle's driver with that machine -- LostOracle extends tests/place_localize_ref.py's PlaceOracle (and through it
tests/localize_ref.py's LocalizeOracle), neither of which is touched.

The rule, per scan that reaches registration (LidarOdometry.h says the same):

  1. the state the scan arrives in is what its record shows as `lost`;
  2. a pending relocalization request is served as before.  The driver's own request counts as an attempt; an accepted request of
     anyone is TRACKING with both streaks at zero; a failed own request is cleared, and the next one is due so that it is served
     retry_every_n_scans scans after this one (a failed caller's request stays pending, as before);
  3. after the gate of an alignment that ran on a scan that did not restart the map: a rejected one extends the bad streak and ends
     the good one, and at bad_scans_to_lost the driver is LOST, remembers the last good pose and owes the first attempt at once; a
     good one ends the bad streak, and while LOST bad_scans_to_lost good ones in a row are TRACKING again;
  4. while the driver is LOST after step 3 the scan goes neither into the local map (nor its key-frame list) nor into the key-frame
     store; its pose, motion model and trajectory are what they would have been;
  5. at the end of the scan, while LOST: the retry count runs down by one; with no request of anyone pending, the count at zero and
     max_attempts not reached, a request is placed for the NEXT observation: `near` (around the remembered pose, diag(near_sigma_xy^2,
     near_sigma_xy^2, ., near_sigma_yaw^2, ., .)) or `keyframes`; near_then_keyframes: the first attempt of a loss is near, every
     later one keyframes.  A near attempt whose grid would exceed relocalization.max_candidates is skipped: no request, no work
     and no attempt (max_attempts does not count it); near_then_keyframes goes on to keyframes at once, near looks again
     retry_every_n_scans scans later.  The record's recovery_gave_up says whether the driver is now LOST with max_attempts used up;
  6. the driver's own request that cannot be served at all (the grids around the kept key-frames exceed max_candidates, no key-frame
     with points) is a failed attempt like any other: the record shows the attempt and no search, and last_error keeps the reason.

Test code only; no product code."""
import math

import numpy as np

import place_localize_ref as plr
import score_ref as sr
from oracle import odometry_oracle as oo
from oracle import oracle_c as oc

DEFAULTS = dict(enabled=False, bad_scans_to_lost=3, method="near_then_keyframes", near_sigma_xy=3.0, near_sigma_yaw_deg=15.0,
                retry_every_n_scans=5, max_attempts=0)
NEAR, KEYFRAMES = 1, 2


def options(cfg):
    """the lost_recovery: block of a loaded pipeline (a dict) over the defaults"""
    b = (cfg or {}).get("lost_recovery") or {}
    o = dict(DEFAULTS)
    for k, v in b.items():
        o[k] = oo._b(v) if k == "enabled" else str(v) if k == "method" else float(v) if k.startswith("near_") else int(v)
    return o


class Machine:
    """mola_hip::LostRecovery"""

    def __init__(self, opt=None):
        self.o = dict(DEFAULTS, **(opt or {}))
        self.reset()

    def reset(self):
        self.lost, self.bad_streak, self.good_streak, self.own_pending, self.wait, self.attempts_this_loss = False, 0, 0, 0, 0, 0
        self.near_done = False
        self.times_lost = self.attempts = self.times_recovered = self.skipped = 0

    def gave_up(self):
        return self.lost and self.o["max_attempts"] != 0 and self.attempts_this_loss >= self.o["max_attempts"]

    def caller_requested(self):
        self.own_pending = 0

    def served(self, succeeded, f):
        """-> True: clear the request (the driver's own, failed)"""
        own, self.own_pending = self.own_pending, 0
        if own:
            f["recovery_attempt"] = own
            self.attempts += 1
            self.attempts_this_loss += 1
        if succeeded:
            f["recovery_succeeded"] = own != 0
            if self.lost:
                self.lost = False
                self.times_recovered += 1
            self.bad_streak = self.good_streak = 0
            return False
        if own:
            self.wait = self.o["retry_every_n_scans"]
        return own != 0

    def gate(self, icp_good, f):
        n = self.o["bad_scans_to_lost"]
        if icp_good:
            self.bad_streak = 0
            if self.lost:
                self.good_streak += 1
                if self.good_streak >= n:
                    self.lost, self.good_streak = False, 0
                    self.times_recovered += 1
        else:
            self.bad_streak += 1
            self.good_streak = 0
            if not self.lost and self.bad_streak >= n:
                self.lost, self.attempts_this_loss, self.wait, self.near_done = True, 0, 0, False
                self.times_lost += 1
        f["bad_streak"] = self.bad_streak

    def due(self, request_pending, near_fits=True):
        if not self.lost:
            return 0
        if self.wait > 0:
            self.wait -= 1
        if request_pending or self.wait > 0 or self.gave_up():
            return 0
        m = self.o["method"]
        if not (m == "near" or (m == "near_then_keyframes" and not self.near_done)):
            return KEYFRAMES
        self.near_done = True
        if near_fits:
            return NEAR
        self.skipped += 1               # no request, no work: not an attempt
        if m == "near_then_keyframes":
            return KEYFRAMES
        self.wait = self.o["retry_every_n_scans"]
        return 0

    def placed(self, kind):
        self.own_pending = kind


def fold(opt, scans):
    """scans: [(icp_good or None, outcome, caller_request, near_fits)] -> what host.LostRecovery.scan() answers for each, a request of the caller
    or of the driver being pending from its placement until it is served with success or, the driver's own, at all"""
    m, pending, out = Machine(opt), False, []
    for icp_good, outcome, caller_request, near_fits in scans:
        if caller_request:
            pending = True
            m.caller_requested()
        f = dict(lost=m.lost, recovery_attempt=0, recovery_succeeded=False, bad_streak=m.bad_streak)
        if pending:
            clear = m.served(outcome, f)
            if outcome or clear:
                pending = False
        if icp_good is not None:
            m.gate(icp_good, f)
        kind = m.due(pending, near_fits)
        if kind:
            pending = True
            m.placed(kind)
        out.append(dict(f, recovery_gave_up=m.gave_up(), placed=kind, pending=pending))
    return out, m


class LostOracle(plr.PlaceOracle):
    """the CPU oracle's driver with relocalization requests (PlaceOracle) and the machine above around them"""

    def __init__(self, pipeline_yaml_path=None, n_threads=8, text=None):
        self.m = Machine()
        super().__init__(pipeline_yaml_path, n_threads=n_threads, text=text)
        self.lr = options(self.cfg)
        self.m = Machine(self.lr)
        self.lost_pose = None
        self.last_error = ""

    def reset(self):
        super().reset()
        self.m.reset()
        self.lost_pose = None
        self.last_error = ""

    def relocalize_near_pose(self, mean_ypr, cov):
        super().relocalize_near_pose(mean_ypr, cov)
        self.in_keyframes = False
        self.m.caller_requested()

    def relocalize_in_keyframes(self):
        super().relocalize_in_keyframes()
        self.m.caller_requested()

    def _serve(self, stamp, rec):
        if self.lr["enabled"] and self.m.own_pending:
            try:
                super()._serve(stamp, rec)
            except (AssertionError, ValueError, RuntimeError) as e:   # cannot be served: a failed attempt, and no search in the record
                self.last_error = repr(e)
                rec.update(relocalization_tried=False, relocalized=False, place_tried=False, place_frames=[], place_shifts=[], place_dists=[],
                           reloc_candidates=0, reloc_ranks=[], reloc_best_n_paired=0, reloc_best_quality=0.0)
        else:
            super()._serve(stamp, rec)
        if self.lr["enabled"]:
            if self.m.served(rec["relocalized"], rec):
                self.request, self.in_keyframes = None, False
            rec["bad_streak"] = self.m.bad_streak

    def _near_fits(self):
        thr = self._score_threshold()
        step = self.reloc["step_xy"]
        step = float(step) if step not in (None, "", "~") and float(step) > 0 else thr
        o, n = self.lr, 1
        for sigma, st in ((o["near_sigma_xy"], step), (o["near_sigma_xy"], step), (math.radians(o["near_sigma_yaw_deg"]), math.radians(self.reloc["step_yaw_deg"]))):
            n *= len(sr.axis_nodes(sigma * sigma, st, self.reloc["sigmas"]))
        return n <= self.reloc["max_candidates"]

    def _gate(self, rec):
        if self._gated or not self.lr["enabled"]:
            return
        self._gated = True
        if rec["icp_run"]:
            was = self.m.lost
            self.m.gate(rec["icp_good"], rec)
            if not was and self.m.lost:
                self.lost_pose = self.last_pose.copy()

    def _insert_into_maps(self):
        rec = self.records[-1]
        self._gate(rec)
        if self.lr["enabled"] and self.m.lost:
            self._skipped = True
            return
        super()._insert_into_maps()

    def _register(self, stamp, rec):
        rec.update(lost=self.m.lost if self.lr["enabled"] else False, recovery_attempt=0, recovery_succeeded=False, recovery_gave_up=False,
                   bad_streak=self.m.bad_streak if self.lr["enabled"] else 0)
        self._gated, self._skipped = False, False
        kfs, counter = list(self.kfs), self.removal_counter
        rec = super()._register(stamp, rec)
        if not self.lr["enabled"]:
            return rec
        if not rec["restarted"]:   # (the scan that restarts the map stands outside the streaks)
            self._gate(rec)
        if self.m.lost and rec["icp_run"]:   # not trusted: the local map's key-frame list is as it was
            self.kfs, self.removal_counter = kfs, counter
            if self._skipped:
                rec["map_updated"] = False
        kind = self.m.due(self.request is not None, not self.m.lost or self._near_fits())
        if kind == NEAR:
            o = self.lr
            self.relocalize_near_pose(oc.pose_to_ypr(self.lost_pose), sr.grid_cov(o["near_sigma_xy"], o["near_sigma_xy"], math.radians(o["near_sigma_yaw_deg"])))
        elif kind == KEYFRAMES:
            self.relocalize_in_keyframes()
        if kind:
            self.m.placed(kind)
        rec["recovery_gave_up"] = self.m.gave_up()
        return rec
