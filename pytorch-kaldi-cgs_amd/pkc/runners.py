"""pkc.runners — forward-mode execution on the HIP kernels, outside the training step:
ModuleRunner (an MLP, any row count), ConvRunner (CNN / SincNet), ForwardRunner (run_nn's forward).
Built on pkc.engine (launch stream, split-K pick), which does not import this module;
torch_optimizer lives there, where Engine.optimizer_state_dict calls it, and is re-exported here.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import call, ptr
from .engine import MAX_SPLITS, Engine, _splits, torch_optimizer  # noqa: F401
from .graph import (TENSOR_OPS, _f32, conv_args, conv_post_args, pattern_effective_masks,
                    resolve_concat, sinc_args, sinc_bind)


def _input_norm_bufs(norms, max_rows, inp_dim, dev):
    """Work buffers of the forward runners' input LayerNorm / BatchNorm (one set per norm)."""
    return [dict(y=_f32(max_rows * inp_dim, dev), xh=_f32(max_rows * inp_dim, dev),
                 st=_f32(2 * max_rows, dev), sm=_f32(inp_dim, dev), si=_f32(inp_dim, dev),
                 work=_f32(L.lib().pkc_dense_work_size(max_rows, inp_dim), dev))
            for _ in norms]


def _run_input_norms(norms, nbufs, cur, cld, K0, M, train, s):
    """ln0 then bn0 of a forward runner over the (M, K0) matrix at address cur (row stride cld);
    returns the address of the normalised matrix (cur itself without norms)."""
    for ns, nb in zip(norms, nbufs):
        if cld != K0:
            raise NotImplementedError("input normalisation of a strided feature stream")
        if ns["kind"] == "ln":
            call("pkc_layernorm_fwd", M, K0, 1, C.c_void_p(cur), 0, None, ptr(ns["gamma"]),
                 ptr(ns["beta"]), C.c_float(1e-6), ptr(nb["y"]), ptr(nb["xh"]), ptr(nb["st"]), s)
        else:
            a = L.DenseFwdArgs(
                M=M, N=K0, nslab=1, zslab=cur, slab_stride=0, bias=None,
                norm=L.NORM_BN_TRAIN if train else L.NORM_BN_EVAL, gamma=ns["gamma"].data_ptr(),
                beta=ns["beta"].data_ptr(), running_mean=ns["rm"].data_ptr(),
                running_var=ns["rv"].data_ptr(), momentum=0.05, eps=1e-5,
                save_mean=nb["sm"].data_ptr(), save_invstd=nb["si"].data_ptr(), act=0,
                xhat=nb["xh"].data_ptr(), out=nb["y"].data_ptr(), count_n=0)
            call("pkc_dense_fwd", C.byref(a), ptr(nb["work"]), s)
        cur = nb["y"].data_ptr()
    return cur


class ModuleRunner:
    """Forward of one MLP module on the pkc kernels for any row count <= max_rows (MLP.forward for
    stand-alone calls, and the per-utterance forward of run_nn's forward mode)."""

    def __init__(self, net, max_rows, inp_dim):
        net.check_supported()
        self.net, self.rows, self.dev = net, max_rows, next(net.parameters()).device
        self.specs = net.layer_specs()
        self.norms = net.input_norm_specs() if hasattr(net, "input_norm_specs") else []
        self.nbufs = _input_norm_bufs(self.norms, max_rows, inp_dim, self.dev)
        self.bufs = []
        K = inp_dim
        for sp in self.specs:
            N = sp["out"]
            b = dict(z=_f32(MAX_SPLITS * max_rows * N, self.dev), K=K, N=N,
                     xhat=_f32(max_rows * N, self.dev), sm=_f32(N, self.dev),
                     si=_f32(N, self.dev), out=_f32(max_rows * N, self.dev),
                     work=_f32(L.lib().pkc_dense_work_size(max_rows, N), self.dev))
            if sp["ln"]:
                b.update(ly=_f32(max_rows * N, self.dev), lxh=_f32(max_rows * N, self.dev),
                         lst=_f32(2 * max_rows, self.dev))
            if sp["quant"]:
                b["Wq"] = torch.zeros_like(sp["W"])
            if sp["inp_quant"]:
                b["xq"] = _f32(max_rows * K, self.dev)
                b["qwork"] = _f32(256, self.dev)
            self.bufs.append(b)
            K = N
        self.prune_work = None
        self.eff = pattern_effective_masks(net, Engine._stream())
        # the reference re-prunes / re-applies pattern^L on every forward call
        self.prunes = any(sp.get("prune") is not None for sp in self.specs) or bool(self.eff)
        if not self.prunes:          # else refreshed at the top of every run()
            self.refresh()

    def refresh(self):
        """Re-apply HCGS masks / the QuantizeLinear clamp and re-quantise (after weights change)."""
        s = Engine._stream()
        for sp, b in zip(self.specs, self.bufs):
            qb = int(sp["quant"] or 0)
            mask = self.eff.get(id(sp["W"]), sp["mask"])
            if sp.get("prune") is not None:      # mask, then prune (neural_networks.py:256-278)
                if mask is not None:
                    call("pkc_apply_mask", ptr(sp["W"]), ptr(mask), sp["W"].numel(),
                         C.c_float(0.0), s)
                if self.prune_work is None:
                    self.prune_work = torch.zeros(L.lib().pkc_prune_work_size(), dtype=torch.uint8,
                                                  device=self.dev)
                call("pkc_prune", ptr(sp["W"]), sp["W"].numel(), C.c_double(float(sp["prune"])), None,
                     ptr(self.prune_work), s)
                if qb:
                    call("pkc_apply_mask", ptr(sp["W"]), None, sp["W"].numel(), C.c_float(1.0), s)
            elif mask is not None or qb:
                call("pkc_apply_mask", ptr(sp["W"]), ptr(mask), sp["W"].numel(),
                     C.c_float(1.0 if qb else 0.0), s)
            if qb:
                call("pkc_fakequant_weight", ptr(sp["W"]), ptr(b["Wq"]), sp["W"].numel(), qb, s)

    def run(self, x_ptr, ld, M, train=False, log_prior=None):
        """x_ptr: device address of an (M, ld) fp32 matrix; returns the (M, N) output view.
        With input quantisation on the first layer, self.input_version holds the address of the
        quantised input (the value the reference leaves in the caller's tensor)."""
        assert M <= self.rows
        if self.prunes:
            self.refresh()
        s = Engine._stream()
        cur, cld = x_ptr, ld
        self.input_version = None
        cur = _run_input_norms(self.norms, self.nbufs, cur, cld, self.bufs[0]["K"], M, train, s)
        for li, (sp, b) in enumerate(zip(self.specs, self.bufs)):
            N, K = b["N"], b["K"]
            if sp["inp_quant"]:
                if cld != K:
                    raise NotImplementedError("input quantisation of a strided feature stream")
                call("pkc_fakequant_input", C.c_void_p(cur), ptr(b["xq"]), M * K,
                     int(sp["inp_quant"]), 1, ptr(b["qwork"]), s)
                cur = b["xq"].data_ptr()
                if li == 0:
                    self.input_version = cur
            W = b["Wq"] if sp["quant"] else sp["W"]
            sf = _splits(M, N, K, MAX_SPLITS)
            call("pkc_gemm", L.PREC_FP32, 1, 1, M, N, K, C.c_void_p(cur), cld, ptr(W), K,
                 ptr(b["z"]), N, sf, M * N, s)
            zp, zs, bias = b["z"].data_ptr(), M * N, sp["b"].data_ptr()
            if sp["ln"]:
                call("pkc_layernorm_fwd", M, N, sf, C.c_void_p(zp), zs, C.c_void_p(bias),
                     ptr(sp["ln_gamma"]), ptr(sp["ln_beta"]), C.c_float(1e-6), ptr(b["ly"]),
                     ptr(b["lxh"]), ptr(b["lst"]), s)
                zp, zs, bias, sf = b["ly"].data_ptr(), 0, None, 1
            if sp["act"] == "softmax":
                a = L.NllArgs(M=M, N=N, nslab=sf, zslab=zp, slab_stride=zs,
                              bias=bias, labels=None, label_stride=0, weight=0.0,
                              logp=b["out"].data_ptr(),
                              log_prior=log_prior.data_ptr() if log_prior is not None else None,
                              dlogits=None, row_loss=None, row_err=None)
                call("pkc_nll_fused", C.byref(a), s)
            else:
                a = L.DenseFwdArgs(
                    M=M, N=N, nslab=sf, zslab=zp, slab_stride=zs, bias=bias,
                    norm=(L.NORM_BN_TRAIN if train else L.NORM_BN_EVAL) if sp["bn"] else L.NORM_NONE,
                    gamma=sp["gamma"].data_ptr(), beta=sp["beta"].data_ptr(),
                    running_mean=sp["rm"].data_ptr(), running_var=sp["rv"].data_ptr(), momentum=0.05,
                    eps=1e-5, save_mean=b["sm"].data_ptr(), save_invstd=b["si"].data_ptr(),
                    act=L.ACT[sp["act"]], drop_p=0.0, seed=0, step_ctr=None, stream_id=0,
                    keep_in=None, keep_out=None, xhat=b["xhat"].data_ptr(), out=b["out"].data_ptr(),
                    count_n=0)
                call("pkc_dense_fwd", C.byref(a), ptr(b["work"]), s)
            cur, cld = b["out"].data_ptr(), N
        return self.bufs[-1]["out"][:M * self.bufs[-1]["N"]].view(M, -1)

    def forward(self, x, train=False):
        x = x.contiguous().float()
        return self.run(x.data_ptr(), x.shape[1], x.shape[0], train).clone()


class ConvRunner:
    """Forward of one CNN / SincNet module on the pkc kernels for any row count <= max_rows
    (run_nn's forward mode): the ModuleRunner interface.  A sinc layer's filters are generated once
    per call."""

    def __init__(self, net, max_rows, inp_dim):
        net.check_supported()
        self.net, self.rows, self.dev = net, max_rows, next(net.parameters()).device
        self.specs = net.conv_specs()
        self.norms = net.input_norm_specs()
        self.nbufs = _input_norm_bufs(self.norms, max_rows, inp_dim, self.dev)
        self.inp_dim = inp_dim
        self.bufs = []
        for sp in self.specs:
            if sp.get("sinc") is not None:
                sinc_bind(sp)
            N = sp["C_out"] * sp["L_out"]
            self.bufs.append(dict(
                N=N, z=_f32(max_rows * N, self.dev), out=_f32(max_rows * N, self.dev),
                off=torch.zeros(max_rows * N, dtype=torch.uint8, device=self.dev),
                xhat=_f32(max_rows * N, self.dev), sm=_f32(sp["C_out"], self.dev),
                si=_f32(sp["C_out"], self.dev), st=_f32(2 * max_rows * sp["C_out"], self.dev)))
        self.input_version = None

    def run(self, x_ptr, ld, M, train=False, log_prior=None):
        assert M <= self.rows
        s = Engine._stream()
        cur, cld = x_ptr, ld
        cur = _run_input_norms(self.norms, self.nbufs, cur, cld, self.inp_dim, M, train, s)
        for sp, b in zip(self.specs, self.bufs):
            if sp.get("sinc") is not None:          # the filters of the current parameters
                call("pkc_sinc_filters_fwd", C.byref(sinc_args(sp)), s)
            a = conv_args(sp, M, cur, cld, b["z"], b["off"])
            call("pkc_conv1d_fwd", C.byref(a), s)
            pa = conv_post_args(sp, M, b["z"], train, b["out"], save_mean=b["sm"].data_ptr(),
                                save_invstd=b["si"].data_ptr(), ln_stat=b["st"].data_ptr(),
                                drop_p=0.0, xhat=b["xhat"].data_ptr())
            call("pkc_conv_post_fwd", C.byref(pa), s)
            cur, cld = b["out"].data_ptr(), b["N"]
        return self.bufs[-1]["out"][:M * self.bufs[-1]["N"]].view(M, -1)

    def forward(self, x, train=False):
        x = x.contiguous().float()
        return self.run(x.data_ptr(), x.shape[1], x.shape[0], train).clone()


class ForwardRunner:
    """run_nn forward mode (core.py:134-145, 234-249) for feed-forward models: one utterance per
    batch, BatchNorm with running statistics, no dropout, posteriors normalised by the log prior.
    The [model] tensor operations (utils.py:2014-2043) run as one pkc_combine_fwd per line; the
    prior of a combine output, and of a head that also feeds a combine, is subtracted on the host
    (core.py:242-245), so the combine reads the head's unnormalised log posteriors."""

    def __init__(self, nets, lines, fea_cols, forward_outs, max_rows=4096):
        fea_cols = resolve_concat(lines, fea_cols)
        self.lines, self.fea_cols, self.outs = lines, fea_cols, forward_outs
        self.nets = nets
        self.max_rows = max_rows
        self.runners = {}
        dims = {k: c1 - c0 for k, (c0, c1) in fea_cols.items()}
        self.combine = {}                      # out -> (op, operand names, constant, N, buffer)
        self.tensor_inputs = set()
        for out, op, a, b in lines:
            if op == "compute":
                runner = ConvRunner if hasattr(nets[a], "conv_specs") else ModuleRunner
                self.runners[a] = runner(nets[a], max_rows, dims[b])
                dims[out] = nets[a].out_dim
            elif op in TENSOR_OPS and out not in fea_cols and a in dims:
                if a in fea_cols and op != "concatenate":
                    raise NotImplementedError(
                        "%s=%s(%s,%s): a feature stream as the first argument of %s is not on "
                        "the pkc path (utils.py:1827-1828, 1907-1920)" % (out, op, a, b, op))
                const = op in ("sum_constant", "mult_constant")
                names = (a,) if const else (a, b)
                if not const and b not in dims:
                    raise ValueError("input %s of %s=%s is neither a feature nor a produced "
                                     "output" % (b, out, op))
                if op != "concatenate" and not const and dims[a] != dims[b]:
                    raise NotImplementedError("%s=%s: operands %d and %d wide (only concatenate "
                                              "takes unequal widths)" % (out, op, dims[a], dims[b]))
                dims[out] = dims[a] + dims[b] if op == "concatenate" else dims[a]
                dev = next(next(iter(nets.values())).parameters()).device
                self.combine[out] = (op, names, float(b) if const else 0.0, dims[out],
                                     _f32(max_rows * dims[out], dev))
                self.tensor_inputs.update(names)
        self.priors_dev = {}

    def forward(self, feats, beg, end, priors):
        M = end - beg
        if M > self.max_rows:
            raise ValueError("utterance of %d frames exceeds the forward buffer" % M)
        produced, res, cur = {}, {}, {}
        for out, op, a, b in self.lines:
            if out in self.combine:
                op, names, c, N, buf = self.combine[out]
                ops = []
                for name in names:
                    if name in cur:
                        raise NotImplementedError("%s: an operand of a combine operation under "
                                                  "in-place input quantisation" % name)
                    if name in self.fea_cols:
                        c0, c1 = self.fea_cols[name]
                        ops.append((feats.data_ptr() + 4 * (beg * feats.stride(0) + c0),
                                    feats.stride(0), c1 - c0))
                    else:
                        ops.append((produced[name].data_ptr(), produced[name].shape[1],
                                    produced[name].shape[1]))
                ca = L.CombineArgs(op=L.COMBINE[op], M=M, Na=ops[0][2],
                                   Nb=ops[1][2] if len(ops) > 1 else 0, a=ops[0][0], lda=ops[0][1],
                                   b=ops[1][0] if len(ops) > 1 else None,
                                   ldb=ops[1][1] if len(ops) > 1 else 0, c=c, out=buf.data_ptr())
                call("pkc_combine_fwd", C.byref(ca), Engine._stream())
                produced[out] = buf[:M * N].view(M, N)
                if out in self.outs:
                    res[out] = produced[out].cpu().numpy()
                    if out in priors:              # core.py:242-245, host side as there
                        res[out] = res[out] - priors[out]
                if all(o in res for o in self.outs):
                    break
                continue
            if op != "compute":
                continue
            if b in cur:                       # the version an earlier consumer quantised in place
                xp, ld = cur[b]
            elif b in self.fea_cols:
                c0, _ = self.fea_cols[b]
                xp, ld = feats.data_ptr() + 4 * (beg * feats.stride(0) + c0), feats.stride(0)
            else:
                xp, ld = produced[b].data_ptr(), produced[b].shape[1]
            lp = None
            host_prior = out in self.tensor_inputs     # a combine reads the unnormalised head
            if out in self.outs and out in priors and not host_prior:
                if out not in self.priors_dev:
                    self.priors_dev[out] = torch.from_numpy(priors[out]).to(feats.device)
                lp = self.priors_dev[out]
            y = self.runners[a].run(xp, ld, M, train=False, log_prior=lp)
            if self.runners[a].input_version is not None:
                cur[b] = (self.runners[a].input_version, ld)
            produced[out] = y
            if out in self.outs:
                res[out] = y.cpu().numpy()
                if host_prior and out in priors:
                    res[out] = res[out] - priors[out]
            if all(o in res for o in self.outs):
                break
        return res
