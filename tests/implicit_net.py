"""Plain numpy restatement of the IGR repository's ``ImplicitNet`` (TEST INFRASTRUCTURE), for arbitrary
``(d_in, dims, skip_in, beta = 100)``, written from its published definition as oracle/igr_oracle.py was:

    dims = [d_in] + dims + [1];  layer l maps dims[l] -> dims[l + 1], or -> dims[l + 1] - d_in when l + 1 is in skip_in
    forward:  x = input;  for every layer l:  if l in skip_in: x = cat([x, input]) / sqrt(2);  x = lin_l(x);
              Softplus(beta, threshold 20) after every layer but the last
    geometric initialisation (Atzmon & Lipman 2020): hidden layers N(0, 2 / out), bias 0; the last layer
    N(sqrt(pi) / sqrt(in), 1e-5), bias -radius_init

``d_in`` counts the whole input, latent code first: [latent, xyz].  Every function takes ``dtype`` so that the same
statement runs in float64 and in np.longdouble (the tests measure float64's own error against the latter).
Trained weights of either shape space are not available offline; the tests run on seeded geometric-init weights.
"""
import numpy as np

BOB_SPOT = dict(d_in=5, dims=[128] * 8, skip_in=(4,))      # IGR_data/train_configs/bob_spot_setup.conf: latent 2
SHAPENET = dict(d_in=7, dims=[256] * 8, skip_in=(4,))      # IGR_data/train_configs/shapenet.conf: latent 4


def layer_dims(d_in, dims, skip_in):
    full = [d_in] + list(dims) + [1]
    return [(full[l + 1] - d_in if l + 1 in skip_in else full[l + 1], full[l]) for l in range(len(full) - 1)]


def geometric_init(seed=0, radius_init=1.0, d_in=5, dims=(128,) * 8, skip_in=(4,)):
    """(Ws, bs): weight[out, in] and bias[out] per layer, seeded numpy."""
    r = np.random.default_rng(seed)
    shapes = layer_dims(d_in, dims, skip_in)
    Ws, bs = [], []
    for l, (out, inp) in enumerate(shapes):
        if l == len(shapes) - 1:
            Ws.append(r.normal(np.sqrt(np.pi) / np.sqrt(inp), 1e-5, (out, inp))); bs.append(np.full(out, -radius_init))
        else:
            Ws.append(r.normal(0.0, np.sqrt(2) / np.sqrt(out), (out, inp))); bs.append(np.zeros(out))
    return Ws, bs


def softplus(z, beta=100.0):
    bz = beta * z
    lin = bz > 20.0
    c = np.minimum(bz, 20.0)
    h = np.where(lin, z, np.log1p(np.exp(c)) / beta)
    dh = np.where(lin, 1.0, 1.0 / (1.0 + np.exp(-c)))
    return h, dh


def _mm(a, w):
    """a [n, in] @ w[out, in].T -> [n, out] (einsum: numpy's matmul has no fast path for long double)."""
    return a @ w.T if a.dtype == np.float64 else np.einsum("ni,oi->no", a, w)


def forward(inp, Ws, bs, skip_in=(4,), beta=100.0, dtype=np.float64, jacobian=True):
    """inp [n, d_in] -> value [n] and (jacobian=True) d value / d input [n, d_in], all in `dtype`.  The derivative is the
    reverse sweep of the same layers (one output: as much work as the forward pass)."""
    inp = np.asarray(inp, dtype)
    Ws = [np.asarray(w, dtype) for w in Ws]
    bs = [np.asarray(b, dtype) for b in bs]
    n, d_in = inp.shape
    s2 = np.sqrt(dtype(2))
    x, slopes = inp, []
    for l in range(len(Ws)):
        if l in skip_in:
            x = np.concatenate([x, inp], 1) / s2
        z = _mm(x, Ws[l]) + bs[l]
        if l < len(Ws) - 1:
            x, dh = softplus(z, dtype(beta))
            slopes.append(dh)
        else:
            x = z
    if not jacobian:
        return x[:, 0]
    g = np.broadcast_to(Ws[-1][0], (n, Ws[-1].shape[1]))      # d value / d (input of the last layer)
    g_inp = np.zeros((n, d_in), dtype)
    for l in range(len(Ws) - 1, -1, -1):
        if l < len(Ws) - 1:
            g = _mm(g * slopes[l], np.ascontiguousarray(Ws[l].T))
        if l in skip_in:
            g_inp = g_inp + g[:, -d_in:] / s2
            g = g[:, :-d_in] / s2
    return x[:, 0], g_inp + g


def query(pts, latent, Ws, bs, skip_in=(4,), dtype=np.float64, jacobian=True):
    """decode_igr's call: input = [latent, xyz].  -> sdf [n], d sdf / d latent [n, L], d sdf / d xyz [n, 3]."""
    pts = np.asarray(pts, dtype)
    latent = np.asarray(latent, dtype).reshape(-1)
    inp = np.concatenate([np.broadcast_to(latent, (len(pts), len(latent))), pts], 1)
    if not jacobian:
        return forward(inp, Ws, bs, skip_in, dtype=dtype, jacobian=False)
    v, J = forward(inp, Ws, bs, skip_in, dtype=dtype)
    return v, J[:, :len(latent)], J[:, len(latent):]


def torch_module(Ws, bs):
    """An ImplicitNet-shaped torch module (lin0 .. lin{n-1}) holding the given layers: what a caller hands to decode_igr."""
    import torch

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for l, (W, b) in enumerate(zip(Ws, bs)):
                lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
                with torch.no_grad():
                    lin.weight.copy_(torch.tensor(W)); lin.bias.copy_(torch.tensor(b))
                setattr(self, "lin%d" % l, lin)
    return Net()
