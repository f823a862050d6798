"""Plain-torch restatement of the reference's CBAM block (networks/equiunet2020.py:147-235 with InstanceNorm3d(1, affine=True)),
evaluated in float64 or float32 on the CPU; gradients come from autograd.  The two maxima are taken the way the reference takes
them -- F.max_pool3d over the whole volume and torch.max(x, 1) -- so their backward follows torch's tie rules (the lowest voxel
index, the lowest channel); amax would split the gradient among equal maxima.

State-dict keys, in order: KEYS.  The eight steps:
  1 avg = mean_v x, mx = max_v x          2 s = sigmoid(mlp(avg) + mlp(mx)), mlp(u) = W2 relu(W1 u + b1) + b2
  3 x1 = x s                                4 comp = [max_c x1 | mean_c x1]
  5 z = conv3d(comp, Wc, padding 3)         6 zn = gamma (z - mu_n) / sqrt(var_n + 1e-5) + beta (biased variance over the sample)
  7 g = sigmoid(relu(zn))                   8 out = x1 g
"""
import torch
import torch.nn.functional as F

KEYS = ("ChannelGate.mlp.1.weight", "ChannelGate.mlp.1.bias", "ChannelGate.mlp.3.weight", "ChannelGate.mlp.3.bias",
        "SpatialGate.spatial.conv.weight", "SpatialGate.spatial.bn.weight", "SpatialGate.spatial.bn.bias")
EPS = 1e-5


def shapes(c, r=16):
    ch = c // r
    return dict(zip(KEYS, ((ch, c), (ch,), (c, ch), (c,), (1, 2, 7, 7, 7), (1,), (1,))))


def forward(sd, x, parts=None):
    """out [N, C, D, H, W]; parts (a dict) receives zn and x1 for the tests' preconditions."""
    w1, b1, w2, b2, wc, gamma, beta = (sd[k] for k in KEYS)
    n, c = x.shape[:2]
    vol = tuple(x.shape[2:])
    avg = F.avg_pool3d(x, vol, stride=vol).view(n, c)
    mx = F.max_pool3d(x, vol, stride=vol).view(n, c)

    def mlp(u):
        return F.linear(torch.relu(F.linear(u, w1, b1)), w2, b2)

    s = torch.sigmoid(mlp(avg) + mlp(mx)).view(n, c, 1, 1, 1)
    x1 = x * s
    comp = torch.cat((torch.max(x1, 1)[0].unsqueeze(1), torch.mean(x1, 1).unsqueeze(1)), dim=1)
    z = F.conv3d(comp, wc, padding=3)
    mu = z.mean(dim=(2, 3, 4), keepdim=True)
    var = z.var(dim=(2, 3, 4), unbiased=False, keepdim=True)
    zn = (z - mu) / torch.sqrt(var + EPS) * gamma.view(1, 1, 1, 1, 1) + beta.view(1, 1, 1, 1, 1)
    if parts is not None:
        parts["zn"], parts["x1"] = zn.detach(), x1.detach()
    return x1 * torch.sigmoid(torch.relu(zn))


def run(sd, x, dout, dtype=torch.float64, parts=None):
    """-> (out, dx, {key: gradient}) of sum(out * dout), everything evaluated in `dtype` on the CPU."""
    p = {k: sd[k].detach().to("cpu", dtype).clone().requires_grad_(True) for k in KEYS}
    xx = x.detach().to("cpu", dtype).clone().requires_grad_(True)
    out = forward(p, xx, parts)
    out.backward(dout.detach().to("cpu", dtype))
    return out.detach(), xx.grad, {k: p[k].grad for k in KEYS}
