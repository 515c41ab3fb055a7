"""fp64 statement of the tracker's update operator (splat_slam_amd.update_op), written from its equations, and the torch composition of
the same weights under autocast that the GPU tests and scripts/update_op_times.py take as the scale of fp16 arithmetic.

    x1 = relu(conv3(relu(conv1(corr))))                 corr_encoder        196 -> 128 -> 128
    x2 = relu(conv3(relu(conv7(flow))))                 flow_encoder          4 -> 128 -> 64
    u  = [inp | x1 | x2]                                320 channels
    g  = mean_hw(sigmoid(conv1_w(net)) * net)           per (edge, channel)
    z  = sigmoid(conv3_z([net | u]) + conv1_zg(g))
    r  = sigmoid(conv3_r([net | u]) + conv1_rg(g))
    q  = tanh(conv3_q([r * net | u]) + conv1_qg(g))
    net' = (1 - z) * net + z * q
    delta  = conv3(relu(conv3(net')))                   [E,h,w,2]
    weight = sigmoid(conv3(relu(conv3(net'))))          [E,h,w,2]
    a  = mean over the edges of each group of relu(conv3(net')), groups = sorted distinct ii
    b  = relu(conv3(a));  eta = 0.01 * softplus(conv3(b));  upmask = conv1(b)
"""
import torch
import torch.nn.functional as F

ACTS = {"none": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def round_fp16(sd):
    """the values the operator holds: every tensor rounded to fp16"""
    return {k: v.to(torch.float16).to(torch.float32) for k, v in sd.items()}


def conv2d_ref(x, w, b=None, act="none"):
    """fp64 convolution with zero padding (k - 1) / 2 on [B,cin,h,w]"""
    x, w = x.double().cpu(), w.double().cpu()
    y = F.conv2d(x, w, None if b is None else b.double().cpu(), padding=w.shape[-1] // 2)
    return ACTS[act](y)


def segmented_mean(x, ii):
    """x [E,...] -> [K,...]: the mean over the edges of each distinct value of ii, in ascending order of the values"""
    groups = sorted(set(int(i) for i in ii))
    return torch.stack([x[[e for e, i in enumerate(ii) if int(i) == g]].mean(0) for g in groups])


def update_ref(sd, net, inp, corr, flow=None, ii=None):
    """the operator in fp64 on the weights sd (keys of update_op.LAYER_SHAPES) exactly as given; inputs [1,E,C,h,w]"""
    P = {k: v.double().cpu() for k, v in sd.items()}

    def conv(name, x, act="none"):
        return conv2d_ref(x, P[name + ".weight"], P[name + ".bias"], act)

    net, inp, corr = net[0].double().cpu(), inp[0].double().cpu(), corr[0].double().cpu()
    E, _, h, w = net.shape
    flow = torch.zeros(E, 4, h, w, dtype=torch.float64) if flow is None else flow[0].double().cpu()
    x1 = conv("corr_encoder.2", conv("corr_encoder.0", corr, "relu"), "relu")
    x2 = conv("flow_encoder.2", conv("flow_encoder.0", flow, "relu"), "relu")
    u = torch.cat([inp, x1, x2], 1)
    g = (conv("gru.w", net, "sigmoid") * net).mean(dim=(2, 3), keepdim=True)
    z = torch.sigmoid(conv("gru.convz", torch.cat([net, u], 1)) + conv("gru.convz_glo", g))
    r = torch.sigmoid(conv("gru.convr", torch.cat([net, u], 1)) + conv("gru.convr_glo", g))
    q = torch.tanh(conv("gru.convq", torch.cat([r * net, u], 1)) + conv("gru.convq_glo", g))
    net = (1 - z) * net + z * q
    delta = conv("delta.2", conv("delta.0", net, "relu")).permute(0, 2, 3, 1)
    weight = conv("weight.2", conv("weight.0", net, "relu"), "sigmoid").permute(0, 2, 3, 1)
    if ii is None:
        return net[None], delta[None].contiguous(), weight[None].contiguous()
    a = segmented_mean(conv("agg.conv1", net, "relu"), ii.tolist())
    b = conv("agg.conv2", a, "relu")
    eta = 0.01 * F.softplus(conv("agg.eta.0", b))[:, 0]
    return net[None], delta[None].contiguous(), weight[None].contiguous(), eta[None], conv("agg.upmask.0", b)[None]


class TorchUpdate:
    """The same operator as a composition of torch ops with the reference's signature: F.conv2d on fp32 parameters under
    torch.autocast, so every convolution runs in fp16 through the vendor library and every elementwise step follows autocast's
    promotion rules; the segmented mean accumulates in the dtype of its input, as a scatter-add does."""

    def __init__(self, sd, device):
        self.p = {k: v.to(device=device, dtype=torch.float32) for k, v in sd.items()}

    def conv(self, name, x, act="none"):
        w = self.p[name + ".weight"]
        return ACTS[act](F.conv2d(x, w, self.p[name + ".bias"], padding=w.shape[-1] // 2))

    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None):
        with torch.autocast("cuda", enabled=True):
            conv = self.conv
            net, inp, corr = net[0], inp[0], corr[0]
            E, _, h, w = net.shape
            flow = torch.zeros(E, 4, h, w, device=net.device) if flow is None else flow[0]
            x1 = conv("corr_encoder.2", conv("corr_encoder.0", corr, "relu"), "relu")
            x2 = conv("flow_encoder.2", conv("flow_encoder.0", flow, "relu"), "relu")
            u = torch.cat([inp, x1, x2], 1)
            g = (conv("gru.w", net, "sigmoid") * net).mean(dim=(2, 3), keepdim=True)
            z = torch.sigmoid(conv("gru.convz", torch.cat([net, u], 1)) + conv("gru.convz_glo", g))
            r = torch.sigmoid(conv("gru.convr", torch.cat([net, u], 1)) + conv("gru.convr_glo", g))
            q = torch.tanh(conv("gru.convq", torch.cat([r * net, u], 1)) + conv("gru.convq_glo", g))
            net = (1 - z) * net + z * q
            delta = conv("delta.2", conv("delta.0", net, "relu")).permute(0, 2, 3, 1).contiguous()
            weight = conv("weight.2", conv("weight.0", net, "relu"), "sigmoid").permute(0, 2, 3, 1).contiguous()
            if ii is None:
                return net[None], delta[None], weight[None]
            uniq, ix = torch.unique(ii.to(net.device), sorted=True, return_inverse=True)
            a = conv("agg.conv1", net, "relu")
            count = torch.zeros(uniq.shape[0], device=net.device, dtype=a.dtype).index_add_(0, ix, torch.ones_like(ix, dtype=a.dtype))
            a = torch.zeros((uniq.shape[0],) + a.shape[1:], device=net.device, dtype=a.dtype).index_add_(0, ix, a)
            a = a / count[:, None, None, None]
            b = conv("agg.conv2", a, "relu")
            eta = 0.01 * F.softplus(conv("agg.eta.0", b))[:, 0]
            return net[None], delta[None], weight[None], eta[None], conv("agg.upmask.0", b)[None]


def make_inputs(E, h, w, seed, device="cpu", dtype=torch.float32):
    """net in tanh range, inp >= 0, corr ~ N(0, 1), flow within +-64; every value fp16-representable"""
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(1, E, 128, h, w, generator=g))
    inp = torch.relu(torch.randn(1, E, 128, h, w, generator=g))
    corr = torch.randn(1, E, 196, h, w, generator=g)
    flow = (128 * torch.rand(1, E, 4, h, w, generator=g) - 64)
    return tuple(t.to(torch.float16).to(dtype).to(device) for t in (net, inp, corr, flow))
