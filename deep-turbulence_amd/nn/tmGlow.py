"""TM-Glow on the MI355X HIP path.  API mirror of the reference's nn/tmGlow.py
(Encoder :26-186, LSTMCFlowDecoder :188-303, TMGlow :305-509): same constructor signatures, method
names, return structures and state_dict keys, so `main.py` can import this package in place of the
reference's `nn` (put `deep-turbulence_amd/` on sys.path instead of `tmglow/`).

Tensors cross this API as logical NCHW fp32 (any strides); internally everything is NHWC and every
numerical operation is a kernel of libtmglow_hip.so -- there is no eager / CPU fallback.
"""
import os

import torch
import torch.nn as nn

import tmg_hip as H
import tmg_ops as ops
from nn.modules.denseBlock import DenseBlock, drop_features
from nn.modules.flowLSTMBlock import LSTMFLowBlock
from nn.modules.flowUtils import GaussianDiag
from nn.modules.misc import UpsamplingLinear


def _on_input_device(fn):
    """Run a model entry point with its first tensor argument's GPU as the current device: the kernels launch on the current
    device's stream, and the reference lets the model live on any cuda:N (main.py:72 `.to(args.src_device)`)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, x, *a, **k):
        if x.is_cuda and x.device.index != torch.cuda.current_device():
            with torch.cuda.device(x.device):
                return fn(self, x, *a, **k)
        return fn(self, x, *a, **k)
    return wrapped


def _conv3(cin, cout, stride):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False, padding_mode='zeros')


class Encoder(nn.Module):
    """Dense conditioning encoder (reference :53-129).  Produces one conditioning map per flow level
    plus the (mean, log-std) map of the deepest latent, each bilinearly up-sampled by `cglow_upscale`."""

    def __init__(self, in_features, enc_block_layers, growth_rate=4, init_features=48, output_features=8, cond_features=8,
                 cglow_upscale=1, bn_size=8, drop_rate=0., bottleneck=False):
        super().__init__()
        self.first_encoder = nn.Sequential()
        self.first_encoder.add_module('In_conv', _conv3(in_features, init_features // 2, 1))
        self.first_encoder.add_module('In_conv3', _conv3(init_features // 2, init_features, 2))
        blocks, cond_convs = [], []
        self.num_feat = init_features
        for i, num_layers in enumerate(enc_block_layers):
            block = nn.Sequential()
            if i > 0:
                trans = nn.Sequential()
                trans.add_module('conv1', _conv3(self.num_feat, self.num_feat // 2, 2))
                if drop_rate > 0:
                    trans.add_module('dropout1', nn.Dropout3d(p=drop_rate))   # reference :183-184
                block.add_module('encode_conv{}'.format(i), trans)
                self.num_feat = self.num_feat // 2
            block.add_module('encode_dense_block{}'.format(i),
                             DenseBlock(num_layers=num_layers, in_features=self.num_feat, bn_size=bn_size, growth_rate=growth_rate,
                                        drop_rate=drop_rate, bottleneck=bottleneck))
            blocks.append(block)
            self.num_feat = self.num_feat + num_layers * growth_rate
            cond_convs.append(nn.Sequential(_conv3(self.num_feat, cond_features, 1)))
        self.out_conv = nn.Sequential(_conv3(self.num_feat, 2 * output_features, 1))
        self.enc_up_scale = UpsamplingLinear(scale_factor=cglow_upscale)
        self.encoding_blocks = nn.ModuleList(blocks)
        self.cond_convs = nn.ModuleList(cond_convs)

    def run(self, xn):
        """NHWC in, NHWC out: (latent map, [conditioning map per level])."""
        fe = self.first_encoder
        out = ops.conv([xn], fe.In_conv.weight)
        out = ops.conv([out], fe.In_conv3.weight, stride=2, relu_in=True)
        up = self.enc_up_scale.scale_factor
        c_out = []
        for i, block in enumerate(self.encoding_blocks):
            mods = list(block._modules.values())
            if i > 0:
                out = drop_features(mods[0], ops.conv([out], mods[0].conv1.weight, stride=2, relu_in=True), 'dropout1')
            out = mods[-1].run(out)
            c0 = ops.conv([out], self.cond_convs[i][0].weight)
            c_out.append(ops.UpsampleFn.apply(c0, up))
        z = ops.UpsampleFn.apply(ops.conv([out], self.out_conv[0].weight), up)
        return z, c_out

    def forward(self, x):
        z, c_out = self.run(H.nhwc(x))
        return H.nchw(z), [H.nchw(c) for c in c_out]


class LSTMCFlowDecoder(nn.Module):
    """Stack of flow levels (reference :210-303)."""

    def __init__(self, in_features, glow_block_layers, cond_features=8, rec_features=8, squeeze_factor=2, conv_ksize=3,
                 LUdecompose=False, train_sampling=True, squeeze_type=0):
        super().__init__()
        self.flow_blocks = nn.ModuleList()
        self.num_feat = in_features
        for num_layers in glow_block_layers:
            self.flow_blocks.append(LSTMFLowBlock(self.num_feat, cond_features, rec_features, num_layers, LUdecompose=LUdecompose,
                                                  train_sampling=train_sampling, do_split=True, squeeze_type=squeeze_type))
            self.num_feat = (self.num_feat * squeeze_factor ** 2) // 2

    def forward(self, x, c_in, h_in, return_eps=False):
        assert (len(c_in) == len(self.flow_blocks)), 'List of conditions need to be same length as flow blocks.'
        z, lds, eps, s_out = x, [], [], []
        for i, flow_block in enumerate(self.flow_blocks):
            z, ld, s0, eps0 = flow_block.forward(z, c_in[i], None if h_in is None else h_in[i], return_eps)
            lds.append(ld)
            eps.append(eps0)
            s_out.append(s0)
        return z, ops.sum_logdet(lds, z.shape[0], z.device), s_out, eps

    def reverse(self, z, c_in, h_in, eps, nonce=None, rows_per_key=None):
        """nonce: key of the in-kernel latent draws of this call (TMGlow.sample); None: every split draws its own.  rows_per_key:
        nonce is a [K, 2] key table and rows m * rows_per_key .. draw with row m (TMGlow.sampleEnsemble)."""
        assert (len(c_in) == len(self.flow_blocks)), 'List of conditions need to be same length as flow blocks.'
        x, lds, s_out = z, [], []
        for i in range(len(self.flow_blocks) - 1, -1, -1):
            rng = None
            if nonce is not None and eps[i] is None:
                rng = (nonce, i) if rows_per_key is None else (nonce, i, rows_per_key)
            x, ld, s0 = self.flow_blocks[i].reverse(x, c_in[i], None if h_in is None else h_in[i], eps[i], rng=rng)
            lds.append(ld)
            s_out.insert(0, s0)
        return x, ops.sum_logdet(lds, x.shape[0], x.device), s_out


class TMGlow(nn.Module):
    """Transient multi-fidelity Glow (reference :336-509)."""

    def __init__(self, in_features, out_features, enc_blocks, glow_blocks, cond_features=8, cglow_upscale=1, growth_rate=4,
                 init_features=48, rec_features=8, bn_size=8, drop_rate=0, bottleneck=False):
        super().__init__()
        self.glow_blocks = glow_blocks
        self.rec_features = rec_features
        enc_out_features = out_features * (2 ** len(glow_blocks))
        self.encoder = Encoder(in_features, enc_block_layers=enc_blocks, growth_rate=growth_rate, init_features=init_features,
                               output_features=enc_out_features, cond_features=cond_features, cglow_upscale=cglow_upscale,
                               bn_size=bn_size, drop_rate=drop_rate, bottleneck=bottleneck)
        self.glow = LSTMCFlowDecoder(out_features, glow_block_layers=glow_blocks, cond_features=cond_features,
                                     rec_features=rec_features, squeeze_factor=2, LUdecompose=True, train_sampling=True,
                                     squeeze_type=0)
        for name in ("in_mu", "in_std", "out_mu", "out_std"):
            self.register_buffer(name, torch.zeros(3))
        print('Total number of parameters: {}'.format(self._num_parameters()))

    def _prior(self, x):
        """(deepest-level prior, conditioning maps): the encoder's [mean | log-std] map goes to the Gaussian kernels as it is
        (reference :399-403 chunks it; the clamp of flowUtils.py:163 is applied inside the kernels)."""
        z, c_out = self.encoder.run(H.nhwc(x))
        return GaussianDiag(hz=z), [H.nchw(c) for c in c_out]

    @_on_input_device
    def forward(self, x, y, h_in=None, return_eps=False):
        """x -> z.  Returns (z, log_prior + log_det [B], h_out, eps | None) (reference :378-414)."""
        cprior, c_out = self._prior(x)
        z, log_det, h_out, eps = self.glow.forward(y, c_out, h_in, return_eps=return_eps)
        if return_eps:
            log_prior, eps0 = cprior.log_prob(z, return_eps=True)
            eps.append(eps0)  # deepest latent noise, from the clamped log-std (reference :407 + flowUtils.py:163)
        else:
            log_prior = cprior.log_prob(z)
            eps = None
        return z, log_prior + log_det, h_out, eps

    @_on_input_device
    def sample(self, x, h_in=None):
        """Conditional generation with freshly drawn latents; no top-prior term in the log-det (reference :417-440)."""
        cprior, c_out = self._prior(x)
        L = len(self.glow_blocks)
        nonce = ops.latent_nonce(x.device)       # one draw from torch's generator keys the in-kernel draws of all L + 1 latents
        z_samp = cprior.sample(rng=(nonce, L))
        eps = [None for _ in range(L)]
        return self.glow.reverse(z_samp, c_out, h_in, eps, nonce=nonce)

    @_on_input_device
    def sampleEnsemble(self, x, h_in, members):
        """`members` samples of the B cases of x in ONE folded call of members * B rows, member-major (row m * B + b: member m, case
        b; h_in holds the states of those rows).  The encoder and the top prior run once for the B cases and their maps are tiled
        to the member rows; member m draws its latents with row m of one latent_nonces table, so it is exactly what a B-row
        sample call keyed by that row computes.  Returns sample's structure for the members * B rows.  Rows are independent only
        in eval mode (BatchNorm on running statistics): the caller sets the mode, as for sample."""
        members = int(members)
        if members < 1:
            raise ValueError("sampleEnsemble needs at least one member, got %d" % members)
        if not x.is_cuda:
            raise RuntimeError("TMGlow.sampleEnsemble runs on the HIP path: the input is on %s (there is no CPU path)" % x.device)
        B = x.shape[0]
        cprior, c_out = self._prior(x)
        L = len(self.glow_blocks)

        def tile(t):                                 # NHWC [B, ...] -> [members * B, ...], member-major
            return t if members == 1 else t.repeat(members, 1, 1, 1)

        c_rep = [H.nchw(tile(H.nhwc(c))) for c in c_out]
        keys = ops.latent_nonces(x.device, members)  # one launch: the keys of all members' L + 1 latents
        z_samp = GaussianDiag(hz=tile(cprior._hz())).sample(rng=(keys, L, B))
        eps = [None for _ in range(L)]
        return self.glow.reverse(z_samp, c_rep, h_in, eps, nonce=keys, rows_per_key=B)

    @_on_input_device
    def reconstruct(self, x, h_in, eps):
        """Generation from given latents, eps[-1] being the deepest (reference :442-467)."""
        cprior, c_out = self._prior(x)
        z_samp = cprior.sample(eps[-1])
        return self.glow.reverse(z_samp, c_out, h_in, eps[:-1])

    def _num_parameters(self):
        return sum(p.numel() for p in self.parameters())

    # ---- seed states ---------------------------------------------------------------------------------------------------------
    # The trainer asks for the seed states of every mini-batch (trainFlowParallel.py:225) and the reference draws them on the host,
    # one generator per (level, sample): 180 M numbers at the metric shape and 64 samples, 1.3 s - twice a 10-step BPTT window on
    # this device.  But the loaders draw the seeds from random_(0, 1000) (dataLoader.py:284, :422): at most 1 000 distinct states
    # exist, 11 MB each at the metric shape, so they live in HBM after their first use and a mini-batch is a device gather.
    # Only seeds below SEED_CACHE_MAX_SEED are admitted: TrainFlow.test and utils.modelPred draw fresh seeds from random_(0, 1e8)
    # for every batch (trainFlowParallel.py:333, utils.py:205) - they never repeat, and caching them would pin 11 MB of HBM per test
    # sample until the budget is full and the training seeds fall back to the host draw.
    SEED_CACHE_GB = float(os.environ.get("TMG_SEED_CACHE_GB", "16"))
    SEED_CACHE_MAX_SEED = 1000

    def _draw_seed_states(self, seed_list, input_dim):
        """The reference's host draw (tmGlow.py:494-509) for the given seeds -> per seed a list over levels of (h, c), [1,R,h,w]."""
        from concurrent.futures import ThreadPoolExecutor
        L = len(self.glow_blocks)

        def draw(job):
            i, seed = job
            gen = torch.Generator().manual_seed(seed)
            dims = [1, self.rec_features, input_dim[0] // (2 ** (i + 1)), input_dim[1] // (2 ** (i + 1))]
            h = 2 * torch.rand(dims, generator=gen) - 1
            return h, torch.randn(dims, generator=gen)

        jobs = [(i, seed) for seed in seed_list for i in range(L)]
        if len(jobs) > 8:
            with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as ex:
                res = list(ex.map(draw, jobs))
        else:
            res = [draw(j) for j in jobs]
        return [res[k * L:(k + 1) * L] for k in range(len(seed_list))]

    def initLSTMStates(self, seeds, input_dim, cache=True):
        """Per (level, sample) a fresh CPU generator with the sample's seed: hidden ~ U[-1,1], cell ~ N(0,1)
        (reference :481-509).  Host RNG by construction (the streams are part of the reference's semantics): every DISTINCT seed is
        drawn once on the host - the (level, sample) draws are independent and run on a small thread pool, torch releases the GIL
        inside rand / randn - and kept on the model's device in the channels-last layout the flow works in; a call is then one
        gather per level.  Returns the reference's structure: a list over levels of (h, c), [B,R,h,w] (values bit-identical to the
        reference's, strides channels-last).  The cache is keyed by (seed, field size), dropped when the model changes device,
        bounded by TMG_SEED_CACHE_GB, and admits only the loaders' seed range [0, SEED_CACHE_MAX_SEED) and only with cache=True;
        every other seed is drawn per call, as in the reference."""
        device = next(self.parameters()).device
        seed_list = [int(s) for s in torch.as_tensor(seeds).tolist()]
        L = len(self.glow_blocks)
        key = (str(device), self.rec_features, int(input_dim[0]), int(input_dim[1]), L)
        cache_ok = bool(cache)
        cache = self.__dict__.get("_seed_states")
        if cache is None or cache["key"] != key:
            cache = {"key": key, "rows": {}, "bytes": 0}
            self.__dict__["_seed_states"] = cache          # (plain attribute: not a buffer, never part of the state_dict)
        rows = cache["rows"]
        missing = [s for s in dict.fromkeys(seed_list) if s not in rows]
        extra = {}
        if missing:
            per_seed = 8 * self.rec_features * sum((input_dim[0] // 2 ** (i + 1)) * (input_dim[1] // 2 ** (i + 1)) for i in range(L))
            for s, lv in zip(missing, self._draw_seed_states(missing, input_dim)):
                # [1,R,h,w] -> [h,w,R] contiguous on the device: stacking such rows gives the flow's NHWC layout directly
                dev_lv = [(h[0].permute(1, 2, 0).contiguous().to(device), c[0].permute(1, 2, 0).contiguous().to(device)) for h, c in lv]
                if cache_ok and 0 <= s < self.SEED_CACHE_MAX_SEED and cache["bytes"] + per_seed <= self.SEED_CACHE_GB * 2 ** 30:
                    rows[s] = dev_lv
                    cache["bytes"] += per_seed
                else:
                    extra[s] = dev_lv
        get = lambda s: rows[s] if s in rows else extra[s]  # noqa: E731
        states = []
        for i in range(L):
            h = torch.stack([get(s)[i][0] for s in seed_list]).permute(0, 3, 1, 2)
            c = torch.stack([get(s)[i][1] for s in seed_list]).permute(0, 3, 1, 2)
            states.append((h, c))
        return states
