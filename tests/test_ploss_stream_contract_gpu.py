"""-m gpu: the stream contract of include/casync_ploss.h ("enqueues on `stream`, allocates nothing and synchronises nothing") and
of calipsync_amd.losses ("on torch's current stream, with no synchronisation"), under the protocol of tests/stream_contract.py:
the call runs on a side stream behind a long row of matrix products, everything it reads is put in place behind them as well,
its results must equal the null-stream run bit for bit and the host must be back while the products are still running.
tests/test_ploss.py closes the header's set of entries on any machine.  Nothing here touches a GPU at import."""
import pytest

import stream_contract as sc

B, H, W = 2, 10, 14
W_PIX, W_PERC = 1.0, 0.1


def _engine():
    import ploss_cases as pc
    from calipsync_amd import losses
    if not hasattr(_engine, "e"):
        _engine.e = losses.PerceptualEngine(pc.state_dict(), sc.DEV)
    return _engine.e


class _Pair(sc.Adapter):
    def make(self, seed):
        import ploss_cases as pc
        pred, label = pc.pair(B, H, W, seed)
        return {"pred": pred, "label": label, "s": sc._t().tensor([1.0 + seed])}

    def inputs(self):
        return {"pred": sc._zeros((B, 3, H, W)), "label": sc._zeros((B, 3, H, W)), "s": sc._zeros((1,))}


class Forward(_Pair):
    """casync_ploss_forward with `saved`, then without, and two forward taps: every buffer the caller's"""
    name = "ploss-forward"
    entries = ("casync_ploss_forward", "casync_ploss_forward_tap")

    def setup(self):
        self.e = _engine()

    def buffers(self):
        torch = sc._t()
        e = self.e
        self.inp = self.inputs()
        self.own = {"scratch": sc._zeros((e.scratch_bytes(B, H, W),), torch.uint8), "saved": sc._zeros((e.saved_bytes(B, H, W),), torch.uint8),
                    "losses": sc._zeros((3,)), "quiet": sc._zeros((3,))}

    def call(self):
        i, o, e = self.inp, self.own, self.e
        e.forward(i["pred"], i["label"], W_PIX, W_PERC, scratch=o["scratch"], saved=o["saved"], losses=o["losses"])
        e.forward(i["pred"], i["label"], 0.0, 1.0, keep=False, scratch=o["scratch"], losses=o["quiet"])
        self.taps = [e.forward_tap(i["pred"], i["label"], s, scratch=o["scratch"]) for s in ("conv2_2", "d")]

    def outputs(self):
        return [self.own["losses"], self.own["saved"], self.own["quiet"]] + self.taps


class Backward(_Pair):
    """casync_ploss_backward and two backward taps on the `saved` of a forward enqueued in front of them on the same stream, the
    scale read from a device scalar that is put in place behind the busy products as well"""
    name = "ploss-backward"
    entries = ("casync_ploss_backward", "casync_ploss_backward_tap")

    def setup(self):
        self.e = _engine()

    def buffers(self):
        torch = sc._t()
        e = self.e
        self.inp = self.inputs()
        self.own = {"scratch": sc._zeros((e.scratch_bytes(B, H, W),), torch.uint8), "saved": sc._zeros((e.saved_bytes(B, H, W),), torch.uint8),
                    "grad": sc._zeros((B, 3, H, W))}

    def call(self):
        i, o, e = self.inp, self.own, self.e
        e.forward(i["pred"], i["label"], W_PIX, W_PERC, scratch=o["scratch"], saved=o["saved"])
        e.backward(i["pred"], i["label"], i["s"], o["saved"], W_PIX, W_PERC, scratch=o["scratch"], out=o["grad"])
        self.taps = [e.backward_tap(i["pred"], i["label"], i["s"], o["saved"], W_PIX, W_PERC, s, scratch=o["scratch"]) for s in ("pool2T", "mask1_1")]

    def outputs(self):
        return [self.own["grad"]] + self.taps


class Training(_Pair):
    """TrainingLoss(preds, labels) and loss.backward(): buffers from torch's allocator, on torch's current stream"""
    name = "training-loss"
    entries = ()

    def setup(self):
        import ploss_cases as pc
        from calipsync_amd import losses
        self.loss = losses.TrainingLoss(state_dict=pc.state_dict(), device=sc.DEV)

    def buffers(self):
        self.inp, self.own = self.inputs(), {}

    def call(self):
        p = self.inp["pred"].detach().clone().requires_grad_(True)
        out = self.loss(p, self.inp["label"])
        (out[0] * self.inp["s"][0]).backward()
        self.res = [o.detach() for o in out] + [p.grad]

    def outputs(self):
        return self.res


ADAPTERS = (Forward, Backward, Training)


@pytest.mark.gpu
@pytest.mark.parametrize("adapter", ADAPTERS, ids=[a.name for a in ADAPTERS])
def test_behind_a_busy_stream(adapter):
    a = adapter()
    assert a.nosync
    sc.run_behind(a)
