"""Several independent optimizee instances stepped by ONE optimizer network, unrolled TOGETHER (round 6).

The reference runs one unroll of one optimizee instance per ``sess.run`` (DM/meta_rnnprop_train.py:397-423,
DM/util.py:31-89); a meta-training batch of optimizees, or BASELINE config 5's replicas, are N such unrolls.  On the
MI355X the neural optimizee (problems.mnist, 784-20-10) has two kernel forms:

    form "chip"  k_mlp_unroll: ONE instance on all 8 XCDs -- the lowest latency of a single unroll
    form "xcd"   k_mlp_xcd:    one instance per XCD, up to 8 per launch -- 3-4 x the throughput

and problems.confocal_microscopy_3d(fused=True), whose batch rows are independent problems, has a third:

    form "rows"  k_cf_unroll:  one workgroup per row of EVERY instance, up to 32 instances of one shape per launch
                               (l2o_confocal_unroll_multi) -- a single instance of batch 32 keeps 32 of the 256 CUs busy.
                               No workgroup waits for another: no snapshot, no status check, no recovery; the results are
                               bit-identical to the instances' own fused launches (which is what form "chip" runs here)

``Replicas`` builds N unroll graphs of one ``MetaOptimizer`` that share its networks and runs them in launches of up to
eight (l2o_mlp_unroll_multi) / 32 (l2o_confocal_unroll_multi) instances, or one after the other on the whole chip:

    reps = Replicas(optimizer, [problems.mnist(...) for _ in range(8)], len_unroll=200)
    reps.reset()
    fx = reps.run({step: 1})            # -> [8] final losses; reps.fx_arrays: the T + 1 losses of every instance
    out = reps.train_step({step: 1}, 1e-3)   # one meta-training step on all of them: the mean of their meta-gradients

Every instance draws its own initial weights and its own minibatches, exactly as N separate ``meta_loss`` graphs would.
"""
from __future__ import annotations

import collections
import os
import warnings

import numpy as np

import torch

from . import _abi
from ._graph_core import _DevGrad, _all_reduce, _world


def _confocal_shape(d):
    """What the instances of one l2o_confocal_unroll_multi launch share (ONE descriptor)."""
    return (int(d.batch), int(d.num_points), tuple(int(r) for r in d.roi), d.img is not None)


def _mismatch(form, inst, first):
    """`inst` cannot ride in the launch that `first` opened (None: the form's fused unroll does not apply to its graph)."""
    if inst is None or inst["net"] is not first["net"]:
        return True
    if form == "rows":
        return _confocal_shape(inst["desc"]) != _confocal_shape(first["desc"])
    return inst["desc"] is not first["desc"]                 # (ONE data set: one descriptor object)


# The forms that run several instances per launch: the graph method that describes one instance, the engine's launch method
# (<multi>_supported answers for a net, a descriptor and an instance count), the instances per launch, the graphs' last_path
# stamp, whether every unroll draws minibatches, and whether the kernel leaves a status word to check (workgroups that wait
# for partner workgroups can time out)
MultiForm = collections.namedtuple("MultiForm", "instance multi per_launch last_path sampled status")
MULTI_FORMS = {
    "xcd": MultiForm("mlp_instance", "mlp_unroll_multi", 8, "mlp_xcd", True, True),
    "rows": MultiForm("confocal_instance", "confocal_unroll_multi", _abi.CONFOCAL_MAX_INSTANCES, "confocal_multi", False, False),
}


class Replicas(object):
    def __init__(self, optimizer, make_losses, len_unroll, net_assignments=None):
        if not make_losses:
            raise ValueError("Replicas needs at least one problem")
        self.optimizer = optimizer
        self.graphs = []
        for make_loss in make_losses:
            g = optimizer._build_graph(make_loss, len_unroll, net_assignments, False)
            if self.graphs:                                  # ONE set of networks for all instances (the first graph's)
                g0 = self.graphs[0]
                if sorted(g.nets) != sorted(g0.nets):
                    raise ValueError("the replicas disagree on the optimizer's networks")
                g.nets = g0.nets
                for s in g.slots:
                    s.net = g0.nets[s.key]
                g._mlp_cache = g0.__dict__.setdefault("_mlp_cache", {})    # (one device copy of the data set)
            self.graphs.append(g)
        optimizer._graph, optimizer._nets = self.graphs[0], self.graphs[0].nets
        self.len_unroll = int(len_unroll)
        self.last_form = None
        self.recoveries = 0
        self.fx_arrays = None

    @property
    def step(self):
        """RNNProp's `step` placeholder (the same object for every replica's feed)."""
        return self.graphs[0].step

    def reset(self):
        for g in self.graphs:
            g.reset()

    def _feed(self, g, feed):
        """`feed` is written against the FIRST graph's placeholders; every replica gets the same values."""
        if not feed:
            return {}
        g0 = self.graphs[0]
        out = {}
        for ph, val in feed.items():
            if ph is g0.step:
                out[g.step] = val
            elif ph in g0.scale:
                raise ValueError("x-scale placeholders are not supported by Replicas")
            else:
                out[ph] = val
        return out

    def _form_supported(self, form, graphs):
        """The engine has the form's kernel, the form's fused unroll applies to every graph in `graphs`, they can share a
        launch, and the library takes the shape for as many instances as a launch would hold."""
        f, eng = MULTI_FORMS[form], self.graphs[0].engine
        if not hasattr(eng, f.multi) or os.environ.get("L2O_DISABLE_FUSED"):
            return False
        first = None
        for g in graphs:
            inst = getattr(g, f.instance)(None, dry=True)
            first = first or inst
            if _mismatch(form, inst, first):
                return False
        return bool(getattr(eng, f.multi + "_supported")(first["net"].spec, first["desc"], min(f.per_launch, len(self.graphs))))

    def xcd_supported(self):
        """Form "xcd" applies to the first replica (run / train_step hold the others against it when they launch)."""
        return self._form_supported("xcd", self.graphs[:1])

    def rows_supported(self):
        """Form "rows" applies: every replica is a problems.confocal_microscopy_3d(fused=True) term of ONE shape whose
        variables are all stepped by one (20, 20) LSTM network, on an engine that has l2o_confocal_unroll_multi."""
        return self._form_supported("rows", self.graphs)

    def _launch_multi(self, form, feed, record=False, who="run"):
        """ENQUEUE one committed unroll of every replica on `form` ("xcd" / "rows"): launches of up to the form's instance
        count, in the replicas' order.  record: the recording kernel, every replica's history into its graph's record plan
        (built once per set of variable buffers).  who: the public method a refusal names.  Returns (instances, per-replica
        records or None)."""
        f, graphs, T = MULTI_FORMS[form], self.graphs, self.len_unroll
        eng = graphs[0].engine
        feed = feed or {}
        kw = {"draw": not self._draw_all()} if f.sampled else {}
        insts = [getattr(g, f.instance)(self._feed(g, feed), **kw) for g in graphs]
        if any(_mismatch(form, i, insts[0]) for i in insts):
            if form == "rows":
                raise _abi.L2OUnsupported(_abi.L2O_ERR_UNSUPPORTED, "Replicas: l2o_confocal_unroll_multi does not apply")
            raise ValueError("Replicas.%s: the replicas must be problems.mnist instances over ONE data set, stepped by one "
                             "(20, 20) LSTM network" % who)
        step0 = int(feed[graphs[0].step]) if graphs[0].rnnprop else 1
        hists = recs = None
        if record:
            hists, recs = [], []
            for g in graphs:
                slots = g.slots
                panels = [v.value.view(*g._panel_shape(v)) for v in g.x]
                plan = g._mlp_hist_plan(T, panels, slots, [s.state for s in slots], [s.m for s in slots], [s.v for s in slots])
                recs.append(dict(step0=step0, shapes=[tuple(p.shape) for p in panels], g=plan["g"], st=plan["st"], m=plan["m"],
                                 v=plan["v"], g_final=plan["g_final"], plan=plan))
                hists.append(plan["hist"])
        net, desc = insts[0]["net"], insts[0]["desc"]
        wpack, launch, n = net.wpack(eng), getattr(eng, f.multi), f.per_launch
        for k in range(0, len(insts), n):
            launch(net.spec, wpack, desc, insts[k:k + n], T, step0, hists=None if hists is None else hists[k:k + n])
        self.last_form = form
        for g in graphs:
            g.last_path = f.last_path
        return insts, recs

    def _record_xcd(self, feed, step0):
        """The forward of a train step on form "xcd" (_launch_multi, recording) as [(record, fx device [T + 1])] per replica;
        step0 is what `feed` says (1 without RNNProp's `step`)."""
        insts, recs = self._launch_multi("xcd", feed, record=True, who="train_step")
        assert all(rec["step0"] == step0 for rec in recs)
        return [(rec, inst["fx"]) for rec, inst in zip(recs, insts)]

    def _draw_all(self):
        """The minibatch indices of ALL replicas in one device draw (one torch generator call instead of one per replica;
        every replica still gets its own independent index sequence) -- when no replica has a host `sampler` and the engine
        draws on the device.  Returns False when the replicas must draw for themselves."""
        graphs = self.graphs
        eng = graphs[0].engine
        if not hasattr(eng, "sample_int") or any(t.hyper.get("sampler") is not None for g in graphs for t in g.terms):
            return False
        from ._graph_core import rng
        d = graphs[0]._mlp_desc(graphs[0].terms[0])
        shape = (len(graphs), self.len_unroll + 1, d.batch)
        big = self.__dict__.get("_idx_all")
        if big is None or tuple(big.shape) != shape:
            big = self._idx_all = eng.empty_int(*shape)
        for j, g in enumerate(graphs):                       # (a graph's reset() drops its index buffers)
            g._mlp_idx = {0: big[j]}
        eng.sample_int(big, d.images.shape[0], int(rng().integers(0, 2 ** 62)))
        return True

    def launch(self, feed=None):
        """ENQUEUE one committed unroll of every replica on the one-instance-per-XCD kernel (launches of up to eight) without
        synchronising the host, without a recovery snapshot and without a status check -- the caller syncs and calls
        engine.check_unroll_status() itself (bench.py's timed region).  Confocal replicas (rows_supported()) go out on
        form "rows" instead, which has no status to check.  Returns the replicas' loss buffers (device, [T + 1])."""
        form = "rows" if self.rows_supported() else "xcd"
        return [i["fx"] for i in self._launch_multi(form, feed, who="launch")[0]]

    def run(self, feed=None, form="auto"):
        """One committed unroll of every replica from its current variables (== N x sess.run([fx, update])).
        form: "xcd" (launches of up to eight instances, one per XCD), "rows" (confocal replicas: launches of up to 32
        instances, one workgroup per row of every instance), "chip" (one instance after the other on the whole chip) or
        "auto" (xcd / rows for two or more replicas where that kernel applies).  Returns the N final losses (host)."""
        if form not in ("auto", "xcd", "rows", "chip"):
            raise ValueError("form must be auto, xcd, rows or chip")
        graphs = self.graphs
        eng = graphs[0].engine
        if form == "rows" or (form == "auto" and len(graphs) > 1 and self.rows_supported()):
            if not self.rows_supported():
                raise _abi.L2OUnsupported(_abi.L2O_ERR_UNSUPPORTED, "Replicas.run(form='rows'): l2o_confocal_unroll_multi does "
                                          "not apply to these optimizees / this network / engine")
            insts, _ = self._launch_multi("rows", feed)
            fx_host = [eng.to_numpy(i["fx"]) for i in insts]    # host sync; nothing to check or to recover from
            self.fx_arrays = fx_host
            return np.array([f[self.len_unroll] for f in fx_host], np.float32)
        use_xcd = form == "xcd" or (form == "auto" and len(graphs) > 1 and self.xcd_supported())
        if use_xcd and not self.xcd_supported():
            raise _abi.L2OUnsupported(_abi.L2O_ERR_UNSUPPORTED, "Replicas.run(form='xcd'): l2o_mlp_unroll_multi does not apply to "
                                      "this optimizee / network / device")
        T = self.len_unroll
        if not use_xcd:
            self.last_form = "chip"
            outs = [g.execute(self._feed(g, feed), True) for g in graphs]
            self.fx_arrays = [o["fx_array"] for o in outs]
            return np.array([o["fx"] for o in outs], np.float32)
        recover = not os.environ.get("L2O_NO_RECOVERY")
        if recover:                                          # (the kernel runs in place and its teams can time out)
            for g in graphs:
                g._arm_snapshot()
        insts, _ = self._launch_multi("xcd", feed)
        if hasattr(eng, "prefetch_unroll_status"):
            eng.prefetch_unroll_status()
        fx_host = [eng.to_numpy(i["fx"]) for i in insts]    # host sync
        try:
            eng.check_unroll_status()
        except _abi.L2OPartnerTimeout as err:
            if not recover:
                raise
            # a team of 32 workgroups did not assemble on its XCD (a masked / shared device): every replica's inputs come
            # back and the unrolls re-run, on the SAME minibatches, on the step-granular kernels
            warnings.warn("open_l2o_amd: %s -- re-running the replicas on the step-granular kernels" % (err,), RuntimeWarning)
            self.recoveries += 1
            fx_host = []
            for g in graphs:
                g._restore_snapshot()
                fx, _ = g._rerun(self._feed(g, feed), True, None, (_abi.OPT_MLP_UNROLL,))
                fx_host.append(eng.to_numpy(fx))
            self.last_form = "steps (recovered)"
            for g in graphs:
                g.last_path = "mlp_xcd"
        self.fx_arrays = fx_host
        return np.array([f[T] for f in fx_host], np.float32)

    # -- meta-training (DM/meta.py:398-414, DM/meta_rnnprop_train.py:559-593) on all replicas at once -----------------------
    def _check_shared(self):
        """The replicas of a train step: problems.mnist over ONE data set -- or problems.confocal_microscopy_3d of ONE
        shape --, all variables stepped by ONE network, without second derivatives."""
        confocal = all(len(g.terms) == 1 and g.terms[0].kind == _abi.PROB_CONFOCAL for g in self.graphs)
        kind, form, what = (_abi.PROB_MLP, "xcd", "the replicas must be problems.mnist instances over ONE data set")
        if confocal:
            kind, form, what = (_abi.PROB_CONFOCAL, "rows",
                                "confocal replicas must be problems.confocal_microscopy_3d instances of ONE shape")
        first = None
        for g in self.graphs:
            g._ensure_init()
            inst = None
            if not g.second_derivatives and len(g.terms) == 1 and g.terms[0].kind == kind \
                    and len({id(s.net) for s in g.slots}) == 1:
                inst = dict(net=g.slots[0].net, desc=g._mlp_desc(g.terms[0]))
            first = first or inst
            if _mismatch(form, inst, first):                 # (the rule of the form's launches, on any engine)
                raise ValueError("Replicas.train_step: %s, stepped by one LSTM network, without second derivatives" % what)

    def _sync_weights(self):
        """Every rank starts from rank 0's network weights (once per Replicas): the meta-gradient is averaged over the
        ranks, so identical weights stay identical."""
        import torch.distributed as dist
        nets = self.graphs[0].nets
        box = [{key: {m: {v: np.asarray(a, np.float32) for v, a in d.items()} for m, d in net.variables.items()}
                for key, net in sorted(nets.items())}]
        dist.broadcast_object_list(box, src=0)
        for key, net in sorted(nets.items()):
            for m, d in box[0][key].items():
                for v, a in d.items():
                    net.assign(m, v, a)

    def train_step(self, feed, learning_rate, form="auto"):
        """One meta-training step on all N replicas, which share the optimizer's networks: loss L = (1/N) sum_r sum_t
        fx_t^r, so the weight gradient is the MEAN of the N single-replica meta-gradients (each what UnrollGraph.train_step
        computes for that replica alone), and ONE Adam step of the optimizer applies it.  Under torch.distributed the
        gradient is also averaged over the ranks (the mean over N x world replicas).
        Forward: launches of up to eight replicas on the recording one-instance-per-XCD kernel where it applies
        (last_form "xcd"), of up to 32 confocal replicas on the recording one-workgroup-per-row kernel (last_form "rows";
        "auto" takes it for two or more replicas), else each replica's own recording unroll (last_form "chip").  Backward:
        the replicas' panels pooled two replicas per BPTT call (the fused BPTT launch takes 8 panels: two MNIST replicas).
        A partner timeout of a recording kernel skips the (device-side, status-guarded) update, takes the Adam step back
        and raises L2OPartnerTimeout, as UnrollGraph.train_step does.
        Returns {"loss": mean over the replicas of sum_t fx_t, "fx": [N] final losses}; fx_arrays as run()."""
        if form not in ("auto", "xcd", "rows", "chip"):
            raise ValueError("form must be auto, xcd, rows or chip")
        graphs = self.graphs
        g0 = graphs[0]
        eng = g0.engine
        T = self.len_unroll
        feed = feed or {}
        for ph in feed:
            if ph in g0.scale:
                raise ValueError("x-scale placeholders are not supported by Replicas")
        self._check_shared()
        rank, world = _world()
        if world > 1 and not self.__dict__.get("_weights_synced"):
            self._sync_weights()
            self._weights_synced = True
        step0 = int(feed[g0.step]) if g0.rnnprop else 1
        use_rows = form == "rows" or (form == "auto" and len(graphs) > 1 and self.rows_supported())
        if use_rows and not self.rows_supported():
            raise _abi.L2OUnsupported(_abi.L2O_ERR_UNSUPPORTED, "Replicas.train_step(form='rows'): "
                                      "l2o_confocal_unroll_multi_record does not apply to these optimizees / this network / engine")
        use_xcd = not use_rows and (form == "xcd" or (form == "auto" and self.xcd_supported()))
        if use_xcd and not self.xcd_supported():
            raise _abi.L2OUnsupported(_abi.L2O_ERR_UNSUPPORTED, "Replicas.train_step(form='xcd'): l2o_mlp_unroll_multi_record "
                                      "does not apply to this optimizee / network / device")
        if use_rows:                                        # (no exchange: no status word guards the update)
            insts, recs = self._launch_multi("rows", feed, record=True, who="train_step")
            runs = [(rec, inst["fx"]) for rec, inst in zip(recs, insts)]
            fused = False
        elif use_xcd:
            runs = self._record_xcd(feed, step0)
            fused = hasattr(eng, "check_unroll_status")
        else:
            self.last_form = "chip"
            runs = []
            for g in graphs:
                rec = {}
                fx, _ = g.launch(self._feed(g, feed), True, record=rec)
                runs.append((rec, fx))
            fused = all(g.last_path in ("fused", "mlp_unroll") for g in graphs) and hasattr(eng, "check_unroll_status")
        # backward: one accumulator per network over all replicas, two replicas per BPTT launch
        out = {}
        sets = [g._bptt_panel_sets(rec) for g, (rec, _) in zip(graphs, runs)]
        caches = self.__dict__.setdefault("_bwd_tables", {})
        for r0 in range(0, len(graphs), 2):
            for key, (net, _) in sets[r0].items():
                panels = [pn for ps in sets[r0:r0 + 2] for pn in ps[key][1]]
                # (the BPTT pointer table of the group: keyed by what it points to -- step 0 of every history buffer)
                ckey = (T,) + tuple(0 if a is None else a.data_ptr() for pn in panels if T
                                    for a in (pn["gs"][0], pn["sts"][0], pn["ms"][0], pn["vs"][0]))
                if ckey not in caches and len(caches) >= 16:
                    caches.pop(next(iter(caches)))
                g0._bptt_panels(net, out.setdefault(key, {}), T, step0, panels, cache=caches.setdefault(ckey, {}))
        srcs = g0.__dict__.get("_gm_src", {})
        n_rep = len(graphs)
        for acc in out.values():                           # the mean: (1/N) sum, then over the ranks
            srcs.pop(id(acc), None)
            keys = sorted(acc)
            flat = torch.cat([acc[k].reshape(-1) for k in keys])
            if n_rep > 1:
                eng.lincomb(flat, flat, 1.0 / n_rep)
            if world > 1:
                _all_reduce(flat)
                eng.lincomb(flat, flat, 1.0 / world)
            off = 0
            for k in keys:
                n = acc[k].numel()
                acc[k] = flat[off:off + n].view(acc[k].shape)
                off += n
        early = all(g0._device_adam(g0.nets[k]) for k in out)
        if early:
            grads = {key: {k: _DevGrad(v) for k, v in acc.items()} for key, acc in out.items()}
        else:
            grads = {key: {k: eng.to_numpy(v) for k, v in acc.items()} for key, acc in out.items()}
        if world > 1 and fused and hasattr(eng, "unroll_status_tensor"):
            # every rank takes the same decision about the meta-step: the status word is MAX-reduced ahead of the guard
            stw = eng.unroll_status_tensor()
            red = torch.zeros(1, dtype=torch.int32, device=eng.device) if stw is None else stw.clone()
            _all_reduce(red, op="MAX")
            if stw is not None:
                stw.copy_(red)
        if early:
            g0._adam_apply(grads, learning_rate, guarded=fused)
        if fused and hasattr(eng, "prefetch_unroll_status"):
            eng.prefetch_unroll_status()                    # (rides on the sync below)
        fx_host = [eng.to_numpy(fx) for _, fx in runs]      # host sync
        if fused:
            g0._guarded_pending = g0.__dict__.get("_guarded_pending", 0) + (1 if early else 0)
            g0._check_unroll_status()                       # raise: the guarded update did not run, its step is taken back
        g0._guarded_pending = 0
        if not early:
            g0._adam_apply(grads, learning_rate)
        self.fx_arrays = fx_host
        return {"loss": np.float32(np.mean([f.sum(dtype=np.float32) for f in fx_host], dtype=np.float32)),
                "fx": np.array([f[T] for f in fx_host], np.float32)}
