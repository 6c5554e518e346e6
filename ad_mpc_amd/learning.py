"""The learning side both fleets share (include/admpc_learn.h, include/admpc_quad_learn.h: observe -> bin -> fit -> install; include/admpc_hyper.h,
include/admpc_quad_hyper.h: search -> re-fit -> install): the
placeholder GPs a fleet that learns is created with, the tensors of the record and the statistics, the fit, the search, and the decode of the
fitted ``AdmpcGp`` records into the dicts ``config.set_gp`` / ``quad_config.set_quad_gp`` take.  ``FleetController`` (fleet.py) and
``QuadFleet`` (quad_fleet.py) derive from ``FleetLearning`` and supply what differs between the vehicles; the search is ``FleetSearch``,
a class of its own on top of it, which ``FleetController`` and ``QuadLearningFleet`` -- what ``QuadFleet(learn=...)`` creates -- derive from."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .config import AdmpcGp, AdmpcGpSearchParams, GP_HYPER, GP_MAX_POINTS, GP_SEARCH_MAX, search_boxes
from .engine import _ptr


def placeholder_gps(learn):
    """The GPs of no points a handle that learns is created with, one per regressor of ``learn``; fit_gp overwrites them on the device."""
    return [dict(feat=d["feat"], out=d["out"], Z=[], alpha=[], length_scale=d["length_scale"], sigma_f=d.get("sigma_f", 1.0)) for d in learn]


def decode_gps(raw, learn, empty):
    """The bytes of len(learn) consecutive AdmpcGp records as the list of dicts set_gp takes.  A record of no features is the placeholder
    of its ``learn`` entry (no fit yet); one with a number that is not finite among those the solve reads is returned as the install
    leaves it in the handle: the empty GP at feature and row ``empty``; otherwise length_scale is the entry's (the fit writes no other
    head than the one given to learn) and Z is [n_points, n_feat]."""
    out = []
    for g, (d, head) in enumerate(zip(learn, placeholder_gps(learn))):
        gp = AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp))
        nf, n = int(gp.n_feat), int(gp.n_points)
        if nf == 0:
            out.append(dict(head, ymean=0.0))
            continue
        Z, alpha = np.ctypeslib.as_array(gp.Z)[:nf, :n].T.copy(), np.ctypeslib.as_array(gp.alpha)[:n].copy()
        nums = np.concatenate(([gp.sigma_f, gp.ymean], gp.inv_l2[:nf], alpha, Z.ravel()))
        if not np.isfinite(nums).all():
            out.append(dict(feat=empty, out=empty, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0))
            continue
        out.append(dict(feat=list(gp.feat[:nf]), out=int(gp.out), Z=Z, alpha=alpha, length_scale=d["length_scale"],
                        sigma_f=float(gp.sigma_f), ymean=float(gp.ymean)))
    return out


class FleetLearning:
    """What a fleet with ``learn`` does besides stepping.  The fleet has ``_eng`` (the controller's handle), ``_nominal``, ``lib``,
    ``device`` and ``B``; its ``_learn`` is None until _alloc_learning."""
    _FIT = _INSTALL = None         # the names of the vehicle's fit and install entries
    _GP_CAP = _REC = _EMPTY = 0    # regressors at most, doubles per sample record, feature and row of the empty GP an install leaves behind
    _NOUN = None                   # what the "does not learn" message calls the fleet

    def _alloc_learning(self, learn, n_gp, obs, prev_shape):
        """The state of a fleet that learns: the regressors, the observe parameters, the latched poses ``_prev``, and the record, the
        statistics and the results of include/admpc_learn.h."""
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
        cap = self._GP_CAP
        self._learn, self.n_learn, self._obs, self._observer = learn, n_gp, obs, self._nominal
        self._prev, self.samples = z(*prev_shape), z(self.B, self._REC)
        self.bins, self.dropped = z(cap, GP_MAX_POINTS, 5), z(cap + 1, dtype=torch.int32)
        self._gp_dev = z(cap * C.sizeof(AdmpcGp), dtype=torch.uint8)
        self.fit_info, self.installed = z(cap, dtype=torch.int32), z(cap, dtype=torch.int32)

    def _learns(self, who):
        if self._learn is None:
            raise ValueError("%s: this %s does not learn, create it with learn=[...]" % (who, self._NOUN))

    def _observe_params(self, who, observing=True):
        """The parameters of an observation or a fit: fixed, unless the vehicle refreshes them."""
        self._learns(who)
        return self._obs

    def _fitted(self):
        """fit_gp has rewritten the records."""

    def _head(self, g, d):
        """The ``learn`` entry whose length_scale and sigma_f learned_gps reports for record g."""
        return d

    def set_observer(self, learned=False):
        """Which handle predicts in observe: the nominal one (default; its residual is what fit_gp has to learn) or the controller's own
        with whatever GPs are installed (what is left of the residual after learning)."""
        self._learns("set_observer")
        self._observer = self._eng if learned else self._nominal

    def observe_reset(self):
        """Forgets every sample: bins and dropped are zeroed on the current stream."""
        self._learns("observe_reset")
        self.bins.zero_()
        self.dropped.zero_()

    def fit_gp(self, min_count=1, install=True):
        """Fits every regressor to the means of its bins with at least `min_count` samples, at the hyperparameters given to ``learn``, and
        (`install`) overwrites the GPs of the controller's handle on the device.  Asynchronous on the current stream; returns the device
        tensors (info int32 [n], installed int32 [n] or None): info[g] is the number of points, or -(k + 1) where pivot k failed and the
        GP is empty; installed[g] is 1 where the record passed the install's check."""
        obs = self._observe_params("fit_gp", observing=False)
        n, s = self.n_learn, self._eng._stream()
        _lib.check(getattr(self.lib, self._FIT)(self._eng.device_index, C.byref(obs), int(min_count), _ptr(self.bins), _ptr(self._gp_dev),
                                               _ptr(self.fit_info), s))
        self._fitted()
        if not install:
            return self.fit_info[:n], None
        _lib.check(getattr(self.lib, self._INSTALL)(self._eng._h, n, _ptr(self._gp_dev), _ptr(self.installed), s))
        return self.fit_info[:n], self.installed[:n]

    def learned_gps(self):
        """The GPs of the last fit_gp (or search_gp, where the fleet has one) as the list of dicts ``set_gp`` / ``set_quad_gp`` /
        ``gp_regressors=`` take (synchronises): to save the model, or to create another handle with what was learned.  length_scale is
        the one given to ``learn`` after a fit_gp, and the one found after a search_gp: the device's own double, from which set_gp forms
        the inv_l2 that was installed.  A record the install refuses (a number that is not finite) is returned as the install leaves it
        in the handle: the empty GP (the car: feature 3, row 3; the quadrotor: feature 7, row 7), no points, mean 0."""
        self._learns("learned_gps")
        torch.cuda.current_stream(self.device).synchronize()
        raw = self._gp_dev.cpu().numpy().tobytes()
        return decode_gps(raw, [self._head(g, d) for g, d in enumerate(self._learn)], self._EMPTY)


def hyper_dicts(hy, bins, n, has_hyper):
    """learned_hyper's list for one block of n regressors: from hy [n, 16] after a search, from the block's given values before."""
    out = []
    for g in range(n):
        b = bins[g]
        nf = int(b.n_feat)
        if not has_hyper:
            out.append(dict(length_scale=[float(b.length[k]) for k in range(nf)], sigma_f=float(b.sigma_f), noise=float(b.noise), nll=float("inf")))
        else:
            out.append(dict(length_scale=[float(hy[g, 10 + k]) for k in range(nf)], sigma_f=float(hy[g, 13]), noise=float(hy[g, 14]),
                            nll=float(hy[g, 15])))
    return out


class FleetSearch(FleetLearning):
    """FleetLearning with the search of the hyperparameters on the device (include/admpc_hyper.h, include/admpc_quad_hyper.h: search ->
    re-fit -> install): what ``FleetController`` (fleet.py) and a ``QuadFleet`` that learns (quad_fleet.py: ``QuadLearningFleet``) share."""
    _SEARCH = _REFIT = None        # the names of the vehicle's search and re-fit entries

    def _alloc_learning(self, learn, n_gp, obs, prev_shape):
        """FleetLearning's state, and the search's: its state per regressor, a scratch of one NLL per candidate, what the last round picked."""
        super()._alloc_learning(learn, n_gp, obs, prev_shape)
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
        cap = self._GP_CAP
        self.hyper, self._nll = z(cap, GP_HYPER), z(cap, GP_SEARCH_MAX)
        self.search_info = z(cap, 2, dtype=torch.int32)
        self._has_hyper = self._searched = False                          # a search has run; _gp_dev holds a re-fit at searched values

    def _fitted(self):
        self._searched = False

    def _head(self, g, d):
        """After a search_gp the length scales and sigma_f it found (the device's own doubles), not those given to ``learn``."""
        if not self._searched:
            return d
        h = self.hyper[g].tolist()
        return dict(d, length_scale=h[10:10 + int(self._obs.gp[g].n_feat)], sigma_f=h[13])

    def search_gp(self, min_count=1, grid=5, rounds=10, shrink=0.5, bounds=None, resume=False, install=True, factor=False):
        """Searches the length scales, sigma_f and the noise of every regressor for the smallest negative log marginal likelihood of its
        points (the bins with at least `min_count` samples), fits at what it found and (`install`) overwrites the GPs of the controller's
        handle on the device: 2 * rounds + 2 launches on the current stream (one more where the search starts), no synchronisation, no allocation.  Every round evaluates
        a regular grid of `grid` points per free slot in the logarithm of the slots, around the best candidate so far, and multiplies
        the grid's step by `shrink`; the first round spans the box.  ``bounds``: config.search_boxes (None: the reference's box;
        lo == hi keeps a slot at that value).  ``resume`` continues the last search on the same statistics with the steps where they
        stand.  Returns the device tensors (info int32 [n] as fit_gp's, or -33 where no candidate had a finite NLL; installed int32
        [n] or None; hyper float64 [n, 16]: the centre's logarithms, the steps, the natural values and the best NLL).  ``factor`` is the
        clustered ensemble's (include/admpc_quad_eval.h: the factors of an evaluation on a log); a fleet without a log refuses it."""
        if factor:
            raise ValueError("search_gp: factor=True needs the clustered ensemble's log (QuadEnsembleFleet, include/admpc_quad_eval.h)")
        obs = self._observe_params("search_gp", observing=False)
        n, dev = self.n_learn, self._eng.device_index
        sp = AdmpcGpSearchParams(grid=int(grid), rounds=int(rounds), shrink=float(shrink), box=search_boxes(self._learn, bounds))
        s = self._eng._stream()
        _lib.check(getattr(self.lib, self._SEARCH)(dev, C.byref(obs), C.byref(sp), int(min_count), 1 if resume else 0, _ptr(self.bins),
                                                  _ptr(self.hyper), _ptr(self._nll), _ptr(self.search_info), s))
        _lib.check(getattr(self.lib, self._REFIT)(dev, C.byref(obs), int(min_count), _ptr(self.bins), _ptr(self.hyper), _ptr(self._gp_dev),
                                                 _ptr(self.fit_info), s))
        self._has_hyper = self._searched = True
        if not install:
            return self.fit_info[:n], None, self.hyper[:n]
        _lib.check(getattr(self.lib, self._INSTALL)(self._eng._h, n, _ptr(self._gp_dev), _ptr(self.installed), s))
        return self.fit_info[:n], self.installed[:n], self.hyper[:n]

    def learned_hyper(self):
        """The hyperparameters of every regressor as the last search_gp left them (synchronises): a list of dicts with length_scale (one
        per feature), sigma_f, noise and nll, the negative log marginal likelihood there.  Before any search: the values given to
        ``learn`` and nll = inf."""
        self._learns("learned_hyper")
        torch.cuda.current_stream(self.device).synchronize()
        return hyper_dicts(self.hyper.cpu().numpy(), self._obs.gp, self.n_learn, self._has_hyper)
