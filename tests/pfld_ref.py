"""Our own restatement of the folded PFLD_GhostOne graph (reference utils/lip_detector/tools/pfld_mobileone.py:99-133 with
every MobileOneBlock as one conv + bias) with torch.nn.functional, dtype-generic; imports nothing of the reference.
tests/test_landmarks.py pins it, together with landmarks.fold, against the reference's own float64 run."""
import torch
import torch.nn.functional as F

from calipsync_amd import landmarks


def forward(folded, x):
    """folded: landmarks.fold(sd, dtype) (numpy, or tensors already on x's device); x [B,3,192,192] tensor (its dtype is the arithmetic's).
    -> (landmarks [B,220], [16 stages, NCHW] in the order of landmarks.STAGES)"""
    f = {k: torch.as_tensor(v).to(device=x.device, dtype=x.dtype) for k, v in folded.items()}
    stages = []

    def block(p, t, stride=1, pad=0, groups=1, act=True):
        t = F.conv2d(t, f[f"{p}.w"], f[f"{p}.b"], stride=stride, padding=pad, groups=groups)
        return F.relu(t) if act else t

    def ghost(p, t, act):
        x1 = block(f"{p}.primary_conv", t, act=act)
        return torch.cat([x1, block(f"{p}.cheap_operation", x1, pad=1, groups=x1.shape[1], act=act)], 1)

    t = block("conv1", x, stride=2, pad=1)
    stages.append(t)
    t = block("conv2", t, pad=1, groups=32)
    stages.append(t)
    means = [t.mean((2, 3))]
    for name, cin, hid, cout, s in landmarks.BOTTLENECKS:
        p = f"{name}.ghost_conv"
        t = ghost(f"{p}.0", t, True)
        if s == 2:
            t = block(f"{p}.1", t, stride=2, pad=1, groups=hid, act=False)
        t = ghost(f"{p}.2", t, False)
        stages.append(t)
        if name in ("conv3_3", "conv4_3", "conv5_4"):
            means.append(t.mean((2, 3)))
    t = block("conv7", t, pad=1)
    stages.append(t)
    x5 = F.relu(F.conv2d(t, f["conv8.w"]))
    stages.append(x5)
    y = F.conv2d(torch.cat(means + [x5.flatten(1)], 1)[:, :, None, None], f["conv_out.w"], f["conv_out.b"]).flatten(1)
    stages.append(y[:, :, None, None])
    return y, stages


def nhwc(t):
    """a stage as the engine taps it"""
    return t.permute(0, 2, 3, 1).contiguous()
