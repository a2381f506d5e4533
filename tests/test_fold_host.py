"""The fold algebra of the IK forward (csrc/fold.h), compiled from the header
into a stand-alone program and run on the host (CPU only): BatchNorm, the gcn
bias times colsum(A) and the residual conv folded into wg / bias2 / wt / biasT
/ wr. Python evaluates the folded form in float64,

    z   = ReLU( mix_A( x . wg'^T ) + bias2 )
    out = ReLU( sum_tap z . wt'_tap^T + res + biasT )

on the oracle's own block input, and compares with the float64 oracle's block
through the comparator of the forward-block tests at margin 1: a float32 fold
evaluated exactly must sit inside the float32 oracle's own rounding noise (the
bar is a property of the reference alone; a missing term is orders of magnitude
over it). Block 0 goes through its data_bn fold from the raw keypoints."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fwdblocks as fb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "temporal_inverse_kinematics_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

WEIGHT_SETS = [("hop2", "std"), ("dense", "hostile"), ("hop2_signed", "std")]
N, T = 2, 9
V = fb.V
BN = ("weight", "bias", "running_mean", "running_var")

# in:  float32 [nblocks], then per block [cin, cout, stride, conv residual?, data_bn?] and its
#      raw tensors in the order of `raw_block` below
# out: per block [mix_sparse, cinp, res] and wg, bias2, amix, wt, biasT (, wr) (, data_bn scale, shift)
SRC = r'''
#include <cstdio>
#include <string>
#include <vector>
#include "fold.h"
using namespace tik_host;
static std::vector<float> in;
static size_t pos = 0;
struct Named { std::string name; std::vector<float> v; };
static void take(std::vector<Named>& t, const std::string& name, size_t n) {
    t.push_back({name, std::vector<float>(in.begin() + pos, in.begin() + pos + n)});
    pos += n;
}
static void take_bn(std::vector<Named>& t, const std::string& pre, size_t n) {
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) take(t, pre + s, n);
}
static void put(FILE* f, const std::vector<float>& v) { fwrite(v.data(), 4, v.size(), f); }
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    fseek(fi, 0, SEEK_END);
    in.resize(ftell(fi) / 4);
    fseek(fi, 0, SEEK_SET);
    if (fread(in.data(), 4, in.size(), fi) != in.size()) return 2;
    fclose(fi);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    const int nb = (int)in[pos++], V = 17;
    for (int b = 0; b < nb; ++b) {
        const int cin = (int)in[pos], cout = (int)in[pos + 1], stride = (int)in[pos + 2], conv = (int)in[pos + 3], dbn = (int)in[pos + 4];
        pos += 5;
        std::vector<float> A(in.begin() + pos, in.begin() + pos + V * V);
        pos += V * V;
        std::vector<Named> t;
        take(t, "gcn.conv.weight", (size_t)cout * cin);
        take(t, "gcn.conv.bias", cout);
        take_bn(t, "tcn.0", cout);
        take(t, "tcn.2.weight", (size_t)cout * cout * 3);
        take(t, "tcn.2.bias", cout);
        take_bn(t, "tcn.3", cout);
        if (conv) {
            take(t, "residual.0.weight", (size_t)cout * cin);
            take(t, "residual.0.bias", cout);
            take_bn(t, "residual.1", cout);
        }
        if (dbn) take_bn(t, "backbone.data_bn", (size_t)V * cin);
        std::vector<tik_tensor> tt;
        for (const Named& n : t) {
            tik_tensor x{};
            x.name = n.name.c_str(); x.data = n.v.data(); x.ndim = 1; x.shape[0] = (int64_t)n.v.size();
            tt.push_back(x);
        }
        TensorMap m;
        FoldedBlock f;
        if (to_map(tt.data(), (int)tt.size(), m) || fold_block(m, "", cin, cout, stride, 1, A, V, f)) {
            fprintf(stderr, "block %d: %s\n", b, g_err.c_str());
            return 1;
        }
        put(fo, {f.mix_sparse ? 1.f : 0.f, (float)f.cinp, (float)f.res});
        put(fo, f.wg); put(fo, f.bias2); put(fo, f.amix); put(fo, f.wt); put(fo, f.biasT);
        if (conv) put(fo, f.wr);
        if (dbn) {
            int C0 = 0;
            std::vector<float> sc, sh;
            if (fold_data_bn(m, V, C0, sc, sh) || C0 != cin) {
                fprintf(stderr, "data_bn: %s\n", g_err.c_str());
                return 1;
            }
            put(fo, sc); put(fo, sh);
        }
    }
    fclose(fo);
    return pos == in.size() ? 0 : 3;
}
'''


def build_program(out_dir, extra_flags=()):
    """hipcc: fold.h + cgemm.hip, whose host code holds the sparse-pattern test the fold calls."""
    src = os.path.join(out_dir, "fold_main.hip")
    with open(src, "w") as f:
        f.write(SRC)
    exe = os.path.join(out_dir, "fold_main")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", *extra_flags,
                        f"-I{CSRC}", src, os.path.join(CSRC, "cgemm.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(str(tmp_path_factory.mktemp("fold")))


def _conv(k):
    ci, co, s = fb.LAYERS[k]
    return ci != co or s != 1


def raw_block(sd, k):
    ci, co, s = fb.LAYERS[k]
    pre = f"backbone.st_gcn_networks.{k}."
    names = ["gcn.conv.weight", "gcn.conv.bias"] + [f"tcn.0.{b}" for b in BN] + ["tcn.2.weight", "tcn.2.bias"] + \
            [f"tcn.3.{b}" for b in BN]
    if _conv(k):
        names += ["residual.0.weight", "residual.0.bias"] + [f"residual.1.{b}" for b in BN]
    parts = [np.array([ci, co, s, _conv(k), k == 0], np.float32),
             (sd["backbone.A"][0] * sd[f"backbone.edge_importance.{k}"][0]).astype(np.float32).ravel()]   # float32 product, as the library forms A_eff
    parts += [np.asarray(sd[pre + n], np.float32).ravel() for n in names]
    if k == 0:
        parts += [np.asarray(sd[f"backbone.data_bn.{b}"], np.float32).ravel() for b in BN]
    return np.concatenate(parts)


def run_fold(exe, graph, kind, work_dir):
    """-> per block, the folded arrays in float64."""
    sd = fb.weights(graph, kind)
    fin, fout = os.path.join(work_dir, f"{graph}_{kind}.in"), os.path.join(work_dir, f"{graph}_{kind}.out")
    np.concatenate([np.array([fb.NL], np.float32)] + [raw_block(sd, k) for k in range(fb.NL)]).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.fromfile(fout, np.float32).astype(np.float64)
    pos, blocks = 0, []

    def take(*shape):
        nonlocal pos
        n = int(np.prod(shape))
        a = o[pos:pos + n].reshape(shape)
        pos += n
        return a
    for k, (ci, co, s) in enumerate(fb.LAYERS):
        sparse, cinp, res = take(3)
        cinp = int(cinp)
        assert cinp == (ci + 3) // 4 * 4 and int(res) == (2 if _conv(k) else 1)
        b = dict(sparse=bool(sparse), wg=take(co, cinp)[:, :ci], bias2=take(V, co), amix=take(V, V), wt=take(co, 3, co), biasT=take(co))
        if _conv(k):
            b["wr"] = take(co, cinp)[:, :ci]
        if k == 0:
            b["bn_sc"], b["bn_sh"] = take(V, ci), take(V, ci)
        blocks.append(b)
    assert pos == o.size
    return blocks


_folded = {}


def folded(program, graph, kind):
    if (graph, kind) not in _folded:
        _folded[graph, kind] = run_fold(program, graph, kind, os.path.dirname(program))
    return _folded[graph, kind]


def eval_folded(b, k, x):
    """Block k's folded form in float64. x: (n,T,V,cin), block 0: the raw keypoints."""
    _, co, s = fb.LAYERS[k]
    if k == 0:
        x = x * b["bn_sc"] + b["bn_sh"]
    y = x @ b["wg"].T                                             # (n,T,V,co)
    z = np.maximum(np.einsum("vw,ntvc->ntwc", b["amix"], y) + b["bias2"], 0.0)
    n, t = z.shape[:2]
    to = (t - 1) // s + 1
    zp = np.zeros((n, t + 2, V, co))
    zp[:, 1:t + 1] = z
    acc = np.zeros((n, to, V, co))
    for tap in range(3):                                          # frame s t' + tap - 1, zero padded
        acc += zp[:, tap:tap + s * (to - 1) + 1:s] @ b["wt"][:, tap].T
    res = x[:, ::s] @ b["wr"].T if "wr" in b else x
    return np.maximum(acc + res + b["biasT"], 0.0).reshape(n, to, V * co)


@functools.lru_cache(maxsize=None)
def block_io(graph, kind, k):
    """(input of block k, the float64 oracle's block k from it), computed once."""
    sd = fb.weights(graph, kind)
    inp = fb.input_kinds(N)[0]
    xin = fb.inputs(inp, N, T) if k == 0 else fb.reference(graph, kind, inp, N, T)[k - 1]
    return xin, fb.block_from_input(sd, k, xin)


@pytest.mark.parametrize("k", range(fb.NL))
@pytest.mark.parametrize("graph,kind", WEIGHT_SETS)
def test_fold_matches_oracle(program, graph, kind, k):
    sd = fb.weights(graph, kind)
    b = folded(program, graph, kind)[k]
    assert b["sparse"] == fb.is_sparse(sd, k)
    xin, ref = block_io(graph, kind, k)
    ci = fb.LAYERS[k][0]
    got = eval_folded(b, k, np.asarray(xin, np.float64).reshape(N, T if k == 0 else xin.shape[1], V, ci))
    ok, err, bar, idx = fb.compare(got, ref, fb.rel32(graph, kind)[k], margin=1.0)
    print(f"fold {graph}/{kind} block {k}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
    assert ok, f"block {k} ({graph}, {kind}): err {err:.3e} > bar {bar:.3e} at {fb.describe(ref, idx, k)}"
