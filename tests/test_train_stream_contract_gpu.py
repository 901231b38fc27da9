"""-m gpu: the stream contract of include/casync_train.h ("Enqueues on `stream`; no upload, no allocation, no workspace, no
synchronisation") and of ``TrainingBatches.batch_for`` ("on torch's current stream and without a synchronisation"), under the
protocol of tests/stream_contract.py: the call runs on a side stream behind a long row of matrix products, everything it reads is
put in place behind them as well, its results must equal the null-stream run bit for bit and the host must be back while the
products are still running.  tests/test_train_data.py closes the header's set of stream-taking entries over ADAPTERS on any
machine.  Nothing here touches a GPU at import."""
import numpy as np
import pytest

import stream_contract as sc
from calipsync_amd.train_data import REC_WORDS, TrainingBatches

H, W, N = 97, 131, 3
# {t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0}: a square, a region cut at both edges, target and reference the same, a 1 x 1 box
REC = np.asarray([(0, 10, 20, 60, 60, 2, 5, 7, 84, 84, 0, 0), (1, 80, 100, 17, 31, 0, 0, 0, 97, 97, 0, 0),
                  (2, 3, 4, 50, 50, 2, 3, 4, 50, 50, 0, 0), (1, 96, 130, 1, 1, 1, 40, 40, 33, 33, 0, 0)], dtype=np.int32)
assert REC.shape[1] == REC_WORDS


class TrainBatchEntry(sc.Adapter):
    """casync_op_train_batch itself: four records over three frames, the records in host memory"""
    name = "train-batch"
    entries = ("casync_op_train_batch",)

    def make(self, seed):
        import kernel_ledger_train
        return {"frames": sc._t().from_numpy(kernel_ledger_train.noise_frames(N, H, W, "stream contract", seed))}

    def buffers(self):
        torch = sc._t()
        self.inp = {"frames": sc._zeros((N, H, W, 3), torch.uint8)}
        self.own = {"img_concat": sc._zeros((len(REC), 6, 160, 160)), "img_real": sc._zeros((len(REC), 3, 160, 160))}

    def call(self):
        sc._ok(sc._lib().casync_op_train_batch(self.inp["frames"].data_ptr(), N, H, W, REC.ctypes.data, len(REC),
                                               self.own["img_concat"].data_ptr(), self.own["img_real"].data_ptr(), sc._stream()),
               "casync_op_train_batch")

    def outputs(self):
        return [self.own["img_concat"], self.own["img_real"]]


class TrainingBatchesFor(sc.Adapter):
    """TrainingBatches.batch_for on a 6-frame 96 x 128 clip with 9 feature steps: the batch kernel, the pinned upload of the window
    indices and the window gather; item 7 shows the last frame"""
    name = "training-batches"
    entries = ()

    def setup(self):
        import frame_data
        from calipsync_amd.resident_clip import ResidentClip
        self.clips = []
        for seed in (0, 1):
            imgs, lms, _ = frame_data.make_frames(6, 96, 128, seed=90 + seed)
            self.clips.append(ResidentClip(imgs, lms, None, sc.DEV))

    def make(self, seed):
        f = np.random.default_rng(95 + seed).standard_normal((9, 2, 1024)).astype(np.float32)
        return {"features": sc._t().from_numpy(f), "frames": self.clips[seed].frames.cpu().clone()}

    def buffers(self):
        self.inp, self.own = {"features": sc._zeros((9, 2, 1024)), "frames": self.clips[0].frames}, {}
        self.loader = TrainingBatches(self.clips[0], self.inp["features"], batch_size=4, seed=0)
        assert self.loader.features.data_ptr() == self.inp["features"].data_ptr()      # a device tensor is taken as it is

    def call(self):
        self.res = list(self.loader.batch_for([3, 0, 7, 2], [1, 4, 0, 6]))

    def outputs(self):
        return self.res

    def close(self):
        for c in getattr(self, "clips", []):
            c.close()


ADAPTERS = (TrainBatchEntry, TrainingBatchesFor)


@pytest.mark.gpu
@pytest.mark.parametrize("adapter", ADAPTERS, ids=[a.name for a in ADAPTERS])
def test_behind_a_busy_stream(adapter):
    a = adapter()
    assert a.nosync
    sc.run_behind(a)
