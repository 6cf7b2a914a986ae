// radiance_grad.hpp — the backward of field_radiance.hpp's radiance field (the harmonic-embedding trunk, the density neuron
// and the colour head of NeuralRadianceFieldFeat in mode="color") with respect to its weights and biases, defined once and
// compiled for host and device.  csrc/radiance_grad.hip holds the kernels and the C entries (include/isr_radiance_grad.h).
//
// One point n = ray * P + k, with the forward's quantities recomputed (the bits of field_radiance.hpp): z_l the chains of the
// hidden layers, h_l = softplus32(z_l), z_o the density neuron's chain, s = softplus32(z_o), z1 the chains of colour layer 1
// (from the ray's direction term), a1 = softplus32(z1), col = sigmoid32(z2); and the upstream values drho = d_densities[n],
// dcol_c = d_colours[n, c]:
//     colour layer 2:   q_c  = dcol_c * (col_c * (1 - col_c))                     (f32 operations in that order)
//                       u1[k] = acc after  acc = fmaf(W2[c,k], q_c, acc)  for c ascending from +0
//     colour layer 1:   g1_j = u1_j * slope32(z1_j, beta)
//     density neuron:   g_o  = (drho * dexp32(s)) * slope32(z_o, beta)
//     into h_top:       u_top[k] = acc after  acc = w_out[k] * g_o (one f32 product), then
//                       acc = fmaf(W1[j,k], g1_j, acc)  for j ascending over Wc, k < Wt only (W1's direction columns produce
//                       no downstream gradient)
//     hidden layers, from the top down:  g_l = u_l * slope32(z_l, beta);
//                       u_{l-1}[k] = acc after  acc = fmaf(W_l[j,k], g_l[j], acc)  for j ascending from +0   (not below layer 0)
// slope32(z, beta) is the derivative of softplus32: sigmoid(beta z) evaluated once in f64 and rounded once, exactly 1 where
// beta z > 20 (softplus32's own threshold, torch's); dexp32(s) = exp(-s), an f64 value rounded once.
// Over the points every gradient is sum_n (output-side factor)[n] * (input-side factor)[n]:
//     dW_l  g_l x h_{l-1} (layer 0: the 6H embedding e);  density row  g_o x h_top;  dW1  g1 x [h_top, e_dir(ray of n)];
//     dW2  q x a1;  every bias: the same output-side factor x 1
// in the order of grad_sums.hpp, the points in memory order.  The direction block of dW1 is summed like every other column,
// e_dir read per ray.  A bias is summed by the f64 policy.
// So a gradient is a function of the inputs, N and P alone.  Origins, directions, lengths and the frequencies get no gradient.
//
// The transposed pack: 64 zero header words, then, each as a matrix-core layer (field_mlp.hpp's w_index) with a zero bias,
//     for every hidden layer l >= 1:  W_l^T     in = O_l rounded up to 32,  out = K_l
//     W1's trunk columns^T:                      in = Wc rounded up to 32,   out = Wt
//     W2^T:                                      in = 32,                    out = Wc
#pragma once
#include "field_radiance.hpp"
#include "grad_sums.hpp"

namespace isr {
namespace radiance {

using grad::kGradChain;      // also the tile of the first kernel
using grad::kGradSlab;
// Points whose block sums the workspace holds at a time: 32 chains x every entry (40 MB for the 256-wide field at H = 60).
constexpr int kGradBatch = 2048;
constexpr int kMaxIn = 6 * kMaxH;       // the widest input of a layer: the embedding

// d softplus32(z, beta) / dz = sigmoid(beta z): one f64 evaluation rounded once; 1 where softplus32 is the identity.
ISR_HD float slope32(float z, float beta) {
  const double t = (double)beta * (double)z;
  if (t > 20.0) return 1.0f;
  return (float)(1.0 / (1.0 + density::exp64(-t)));
}

// exp(-s): what torch's backward of 1 - exp(-s) multiplies by.  NaN gives NaN.
ISR_HD float dexp32(float s) { return (float)density::exp64(-(double)s); }

struct GradLayout {
  int total_words;
  Layer T[density::kMaxHidden];      // T[0] is empty
  Layer trunkT, outT;
};

ISR_HD void make_layout_t(const Layout& lay, GradLayout& t) {
  int off = field::kHeaderWords;
  t.T[0] = Layer{0, 0, 0, 0, 0, off, off};
  for (int l = 1; l < density::kMaxHidden; ++l) {
    if (l < lay.d.n_hidden) field::add_layer(lay.d.L[l].OP, lay.d.L[l].K, 1, off, t.T[l]);
    else t.T[l] = t.T[0];
  }
  field::add_layer(lay.WcP, lay.d.out_K, 1, off, t.trunkT);
  field::add_layer(32, lay.Wc, 1, off, t.outT);
  t.total_words = off;
}

// Where the real entries sit in the standard layout (isr_radiance_pack's W and b): the hidden layers [0, n_hidden), the
// density row [n_hidden], W1 [n_hidden + 1], W2 [n_hidden + 2].
struct StdOffsets {
  int w[density::kMaxHidden + 3], b[density::kMaxHidden + 3];
  int w_total, b_total;
};

ISR_HD void std_offsets(const Layout& lay, StdOffsets& s) {
  int w = 0, b = 0, i = 0;
  for (; i < lay.d.n_hidden; ++i) {
    s.w[i] = w;
    s.b[i] = b;
    w += lay.d.L[i].O * lay.d.L[i].K;
    b += lay.d.L[i].O;
  }
  s.w[i] = w, s.b[i] = b, ++i;
  w += lay.d.out_K, b += 1;
  s.w[i] = w, s.b[i] = b, ++i;
  w += lay.Wc * (lay.d.out_K + 6 * lay.d.H), b += lay.Wc;
  s.w[i] = w, s.b[i] = b, ++i;
  w += lay.C * lay.Wc, b += lay.C;
  for (; i < density::kMaxHidden + 3; ++i) s.w[i] = w, s.b[i] = b;
  s.w_total = w;
  s.b_total = b;
}

// Host: the weights out of a pack, dense and row-major (W[j * K + k])
struct HostNet {
  std::vector<std::vector<float>> W;
  std::vector<float> trunk, out;
  const float* rows[density::kMaxHidden];
  HostNet(const Layout& lay, const void* pack) {
    const float* pf = static_cast<const float*>(pack);
    W.resize(lay.d.n_hidden);
    for (int l = 0; l < lay.d.n_hidden; ++l) {
      W[l].resize((size_t)lay.d.L[l].O * lay.d.L[l].K);
      field::unpack_layer(lay.d.L[l], pf, W[l].data(), false);
      rows[l] = W[l].data();
    }
    trunk.resize((size_t)lay.trunk.O * lay.trunk.K);
    field::unpack_layer(lay.trunk, pf, trunk.data(), false);
    out.resize((size_t)lay.out.O * lay.out.K);
    field::unpack_layer(lay.out, pf, out.data(), false);
  }
};

// Host: e_dir (6H) and the direction term u (Wc) of one ray: the chain from b1 over W1's direction columns
inline void ray_grad_term(const Layout& lay, const void* pack, const float* dirT, const float* dirv, float* e, float* u) {
  const float* pf = static_cast<const float*>(pack);
  float dn[3];
  normalize3(dirv, dn);
  density::embed_point(dn, pf + density::kFreqOff, lay.d.H, e);
  for (int j = 0; j < lay.Wc; ++j) u[j] = pf[lay.dir.b_off + j];
  for (int k = 0; k < 6 * lay.d.H; ++k) {
    const float ek = e[k];
    const float* wk = dirT + (size_t)k * lay.Wc;
    for (int j = 0; j < lay.Wc; ++j) u[j] = fmaf(wk[j], ek, u[j]);
  }
}

// Host: one point.  The forward from x and its ray's direction term `uray`, keeping every layer's input (e, Hh[l], a1) and
// slope, then the rule above from drho and dcol (C values) down: G[l] (O_l), *go, g1 (Wc), q (C).
inline void point_grads(const Layout& lay, const void* pack, const HostNet& net, const float* x, const float* uray, float drho,
                        const float* dcol, float* e, float* const* Hh, float* a1, float* const* G, float* go, float* g1,
                        float* q) {
  const float* pf = static_cast<const float*>(pack);
  const float beta = pf[0];
  const int nh = lay.d.n_hidden, Wt = lay.d.out_K, Wc = lay.Wc, C = lay.C;
  float u[kMaxWidth], v[kMaxWidth];
  density::embed_point(x, pf + density::kFreqOff, lay.d.H, e);
  const float* h = e;
  for (int l = 0; l < nh; ++l) {
    const Layer& L = lay.d.L[l];
    for (int j = 0; j < L.O; ++j) {
      const float* w = net.rows[l] + (size_t)j * L.K;
      float z = pf[L.b_off + j];
      for (int k = 0; k < L.K; ++k) z = fmaf(w[k], h[k], z);
      Hh[l][j] = density::softplus32(z, beta);
      G[l][j] = slope32(z, beta);            // the slope, until the way down replaces it by g
    }
    h = Hh[l];
  }
  {
    float zo = pf[lay.d.out_b_off];
    for (int k = 0; k < Wt; ++k) zo = fmaf(pf[lay.d.out_w_off + k], h[k], zo);
    const float s = density::softplus32(zo, beta);
    *go = (drho * dexp32(s)) * slope32(zo, beta);
  }
  for (int j = 0; j < Wc; ++j) {
    const float* w = net.trunk.data() + (size_t)j * Wt;
    float z = uray[j];
    for (int k = 0; k < Wt; ++k) z = fmaf(w[k], h[k], z);
    a1[j] = density::softplus32(z, beta);
    g1[j] = slope32(z, beta);
  }
  for (int c = 0; c < C; ++c) {
    const float* w = net.out.data() + (size_t)c * Wc;
    float z = pf[lay.out.b_off + c];
    for (int k = 0; k < Wc; ++k) z = fmaf(w[k], a1[k], z);
    const float col = sigmoid32(z);
    q[c] = dcol[c] * (col * (1.0f - col));
  }
  for (int k = 0; k < Wc; ++k) {
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc = fmaf(net.out[(size_t)c * Wc + k], q[c], acc);
    g1[k] = acc * g1[k];
  }
  for (int k = 0; k < Wt; ++k) {
    float acc = pf[lay.d.out_w_off + k] * *go;
    for (int j = 0; j < Wc; ++j) acc = fmaf(net.trunk[(size_t)j * Wt + k], g1[j], acc);
    u[k] = acc;
  }
  for (int l = nh - 1; l >= 0; --l) {
    const Layer& L = lay.d.L[l];
    for (int j = 0; j < L.O; ++j) G[l][j] = u[j] * G[l][j];
    if (l == 0) break;
    for (int k = 0; k < L.K; ++k) {
      float acc = 0.f;
      for (int j = 0; j < L.O; ++j) acc = fmaf(net.rows[l][(size_t)j * L.K + k], G[l][j], acc);
      v[k] = acc;
    }
    for (int k = 0; k < L.K; ++k) u[k] = v[k];
  }
}

// Host: the whole backward over host arrays.  d_densities / d_colours null: zeros.  dW / db null: not written.
// par(n, per_thread_min, fn) runs fn(i) for i in [0, n), in any order (isr::parallel_rows, or a plain loop).
template <class Par>
void backward_host(const Par& par, const Layout& lay, const void* pack, const float* origins, const float* directions,
                          const float* lengths, int N, int P, const float* d_densities, const float* d_colours, float* dW,
                          float* db) {
  const int nh = lay.d.n_hidden, Wt = lay.d.out_K, Wc = lay.Wc, C = lay.C, E = 6 * lay.d.H;
  const long NP = (long)N * P;
  StdOffsets so;
  std_offsets(lay, so);
  const HostNet net(lay, pack);
  std::vector<float> dirT((size_t)Wc * E);
  field::unpack_layer(lay.dir, static_cast<const float*>(pack), dirT.data(), true);
  std::vector<float> edir((size_t)N * E), ur((size_t)N * Wc);
  par((long)N, 64L, [&](long ray) {
    ray_grad_term(lay, pack, dirT.data(), directions + 3 * ray, edir.data() + ray * E, ur.data() + ray * Wc);
  });
  std::vector<float> e((size_t)NP * E), a1((size_t)NP * Wc), g1((size_t)NP * Wc), q((size_t)NP * C), go((size_t)NP);
  std::vector<std::vector<float>> Hh(nh), G(nh);
  for (int l = 0; l < nh; ++l) {
    Hh[l].resize((size_t)NP * lay.d.L[l].O);
    G[l].resize((size_t)NP * lay.d.L[l].O);
  }
  par(NP, 64L, [&](long n) {
    const long ray = n / P;
    float x[3], dc[kMaxC];
    for (int d = 0; d < 3; ++d) x[d] = origins[3 * ray + d] + directions[3 * ray + d] * lengths[n];
    for (int c = 0; c < C; ++c) dc[c] = d_colours ? d_colours[(size_t)n * C + c] : 0.f;
    float *hp[density::kMaxHidden], *gp[density::kMaxHidden];
    for (int l = 0; l < nh; ++l) {
      hp[l] = Hh[l].data() + (size_t)n * lay.d.L[l].O;
      gp[l] = G[l].data() + (size_t)n * lay.d.L[l].O;
    }
    point_grads(lay, pack, net, x, ur.data() + ray * Wc, d_densities ? d_densities[n] : 0.f, dc, e.data() + (size_t)n * E, hp,
                a1.data() + (size_t)n * Wc, gp, &go[n], g1.data() + (size_t)n * Wc, q.data() + (size_t)n * C);
  });
  // a row of a gradient matrix (and its bias) at a time
  struct Row {
    int layer, j;
  };
  std::vector<Row> rows;
  for (int l = 0; l < nh; ++l)
    for (int j = 0; j < lay.d.L[l].O; ++j) rows.push_back({l, j});
  rows.push_back({nh, 0});
  for (int j = 0; j < Wc; ++j) rows.push_back({nh + 1, j});
  for (int c = 0; c < C; ++c) rows.push_back({nh + 2, c});
  const float* h_top = Hh[nh - 1].data();
  par((long)rows.size(), 8L, [&](long r) {
    const int l = rows[r].layer, j = rows[r].j;
    const float *g, *hm;
    long gs;
    int K;
    if (l < nh) {
      g = G[l].data() + j, gs = lay.d.L[l].O, K = lay.d.L[l].K;
      hm = l ? Hh[l - 1].data() : e.data();
    } else if (l == nh) {
      g = go.data(), gs = 1, K = Wt, hm = h_top;
    } else if (l == nh + 1) {
      g = g1.data() + j, gs = Wc, K = Wt, hm = h_top;
    } else {
      g = q.data() + j, gs = C, K = Wc, hm = a1.data();
    }
    const int ld = l == nh + 1 ? Wt + E : K;
    if (dW) {
      grad::blocked_row<kMaxIn>(g, gs, hm, K, 1, NP, true, dW + so.w[l] + (size_t)j * ld);
      if (l == nh + 1) grad::blocked_row<kMaxIn>(g, gs, edir.data(), E, P, NP, true, dW + so.w[l] + (size_t)j * ld + Wt);
    }
    if (db) grad::blocked_row<kMaxIn>(g, gs, nullptr, 1, 1, NP, true, db + so.b[l] + j);
  });
}

}  // namespace radiance
}  // namespace isr
