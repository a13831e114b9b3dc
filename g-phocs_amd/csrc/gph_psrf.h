// gph_psrf.h -- the potential scale reduction factor of one trace column over R replicate chains (Gelman & Rubin 1992;
// include/gphocs_hip.h: gph_psrf).  Host code, plain fp64, every sum in the order written:
//   m_r = (sum_s x[r][s], sample order) / S             v_r = (sum_s (x[r][s] - m_r)^2, sample order) / (S - 1)
//   Wv  = (sum_r v_r, chain order) / R                  M   = (sum_r m_r, chain order) / R
//   Bn  = (sum_r (m_r - M)^2, chain order) / (R - 1)    V   = ((double)(S - 1) / (double)S) * Wv + Bn
//   out = {M, sqrt(Wv), sqrt(Bn), sqrt(V / Wv)};  Wv == 0: psrf is 1 if Bn == 0, else +inf
// Included by gph_mcmc.cpp inside its extern "C" block (built with -ffp-contract=off like everything else: no fused V).
int gph_psrf(const double *x, int32_t R, int64_t S, double *out)
{
  if (!x || !out || R < 2 || S < 2) return GPH_EARG;
  double sv = 0.0, sm = 0.0;
  std::vector<double> mean((size_t)R);
  for (int32_t r = 0; r < R; r++) {
    const double *xr = x + (size_t)r * (size_t)S;
    double s = 0.0, ss = 0.0;
    for (int64_t k = 0; k < S; k++) s = s + xr[k];
    const double m = s / (double)S;
    for (int64_t k = 0; k < S; k++) { const double d = xr[k] - m; ss = ss + d * d; }
    mean[(size_t)r] = m;
    sv = sv + ss / (double)(S - 1);
    sm = sm + m;
  }
  const double Wv = sv / (double)R, M = sm / (double)R;
  double sb = 0.0;
  for (int32_t r = 0; r < R; r++) { const double d = mean[(size_t)r] - M; sb = sb + d * d; }
  const double Bn = sb / (double)(R - 1);
  const double V = ((double)(S - 1) / (double)S) * Wv + Bn;
  out[0] = M; out[1] = sqrt(Wv); out[2] = sqrt(Bn);
  out[3] = Wv == 0.0 ? (Bn == 0.0 ? 1.0 : INFINITY) : sqrt(V / Wv);
  return 0;
}
