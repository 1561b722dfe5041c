"""Erasing moving objects from a live local map restated on the CPU oracle, straight from the text of include/molahip_live.h and
of mola_lidar_odometry_hip/LiveMapCleaning.h.  view, vote and decide are tests/clean_ref.py's (numpy); the map is oracle_c.Map;
erasing is dump(), filter, a fresh map of the same parameters and one insert of the kept points in storage order (they are a
subset of what the map held, so the cap and the in-voxel clearance accept every one of them again).  No product code."""
import numpy as np

import clean_ref as cr
from oracle import oracle_c as oc
from oracle.odometry_oracle import OdometryOracle

I12 = np.eye(4)[:3].reshape(12)
HOST_DEFAULT = dict(max_view_distance=30.0, max_views=24, min_through_votes=2, agree_weight=1, every_n_updates=1)


def world_to_view(T_view):
    """nbr_T of a view recorded at pose T_view: the header's relative pose with T_i = identity."""
    return cr.relative_pose(I12, T_view)


def ring_neighbours(ring, T_now, max_view_distance=30.0, **_):
    """The kept slots (ring: slot -> (view, pose)) whose recorded position lies within max_view_distance of T_now, compared as
    cleaning_neighbours does, in ascending slot order."""
    a = np.asarray(T_now, np.float64).reshape(-1)[:12]
    lim = float(max_view_distance) * float(max_view_distance)
    out = []
    for slot in sorted(ring):
        b = np.asarray(ring[slot][1], np.float64).reshape(-1)[:12]
        dx, dy, dz = b[3] - a[3], b[7] - a[7], b[11] - a[11]
        if (dx * dx + dy * dy) + dz * dz <= lim:
            out.append(slot)
    return out


def vote_map(m, views, nbr_view, nbr_T, **params):
    """mh_views_vote_map on an oracle_c.Map: one word per stored point, in dump order."""
    return cr.vote(m.dump()["xyz"], views, nbr_view, nbr_T, **params)


def erase(m, map_args, drop):
    """(the map after mh_map_erase_points, the kept mask)."""
    keep = ~np.asarray(drop, bool)
    xyz = m.dump()["xyz"]
    assert len(keep) == len(xyz)
    out = oc.Map(*map_args)
    if keep.any():
        out.insert(xyz[keep])
        assert out.num_points == int(keep.sum())  # a subset is accepted whole
    return out, keep


class LiveFold:
    """The rule of LiveMapCleaning.h on one oracle map: update(scan, pose) inserts, writes the ring slot and, when due, erases.
    `on_erase(xyz of the stored points, drop mask)` is told about every erasing."""

    def __init__(self, map_args, params=None, host=None, on_erase=None):
        self.map_args = tuple(map_args)
        self.params = dict(cr.DEFAULT, **(params or {}))
        self.host = dict(HOST_DEFAULT, **(host or {}))
        self.map = oc.Map(*self.map_args)
        self.ring = {}
        self.u = 0
        self.erased = 0
        self.on_erase = on_erase

    def clean(self, scan_xyz, T):
        """steps 1 and 2 of the rule, behind this update's insertions"""
        h = self.host
        self.ring[self.u % int(h["max_views"])] = (cr.view(scan_xyz, **self.params), np.array(T, np.float64).reshape(-1)[:12].copy())
        due = (self.u + 1) % int(h["every_n_updates"]) == 0
        self.u += 1
        if not due:
            return False
        slots = ring_neighbours(self.ring, T, **h)
        views = {s: self.ring[s][0] for s in slots}
        votes = vote_map(self.map, views, slots, [world_to_view(self.ring[s][1]) for s in slots], **self.params)
        drop = cr.decide(votes, **h)
        if self.on_erase is not None:
            self.on_erase(self.map.dump()["xyz"], drop)
        self.map, keep = erase(self.map, self.map_args, drop)
        self.erased += int(drop.sum())
        return True

    def update(self, scan_xyz, T, remove_far=0.0):
        self.map.insert_posed(scan_xyz, T, remove_far)
        return self.clean(scan_xyz, T)


class LiveOracle(OdometryOracle):
    """The CPU oracle of the driver with the online_map_cleaning: block enabled (the one-map default chain): every local map
    update is followed by the rule above (clean=False: the plain driver, with the same book-keeping).  ledger (live_cases.Ledger)
    and scan_mover (the mover mask of the scan being fed, over its raw points) are optional book-keeping for the tests."""

    def __init__(self, *a, params=None, host=None, clean=True, ledger=None, **kw):
        self._live_params, self._live_host, self._live_clean = params, host, clean
        self.ledger, self.scan_mover = ledger, None
        super().__init__(*a, **kw)

    def reset(self):
        super().reset()
        self.fold = None

    def _clear_maps(self):
        super()._clear_maps()
        self.fold = None  # (whatever clears the maps empties the ring)

    def _insert_into_maps(self):
        if self.ledger is not None and self.scan_mover is not None:
            self.ledger.offered(self.for_map, self.last_pose, np.asarray(self.scan_mover, bool)[self.idx_map])
        super()._insert_into_maps()
        if not self._live_clean:
            return
        if self.fold is None:
            self.fold = LiveFold(self._map_args, self._live_params, self._live_host,
                                 on_erase=None if self.ledger is None else self.ledger.on_erase)
        self.fold.map = self.map
        self.records[-1]["map_cleaned"] = self.fold.clean(self.for_map, self.last_pose)
        self.map = self.fold.map
