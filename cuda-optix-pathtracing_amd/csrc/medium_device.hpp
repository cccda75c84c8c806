// medium_device.hpp -- the device side of the participating medium (medium.hpp): the per-lane Halton index,
// the free flight, the transmittance of shadow segments and the scatter vertex that path_shade's *_medium rows call.
//
// Part of dmt_hip.hip's translation unit, included once between shade_hit and path_shade.  Nothing here is referenced by a
// kernel instantiated without kFeatMedium.  Under kFeatMediumGrid (the *_medium_grid rows; medium_grid.hpp)
// the extinction is sigmaT times a grid of densities: the free flight and the transmittance come from medium_grid_march.
// Under kFeatMediumSpectrum (the *_rgb rows) sigmaT is the reference channel's extinction, the event at the
// end of a segment is medium_spectrum_event's, and transmittances are taken per channel.
#pragma once

// the distance to the next collision for the number u in [0, 1), and the transmittance over a length
DMT_DEV float medium_free_flight(float sigmaT, float u) { return -log1pf(-u) / sigmaT; }
DMT_DEV float medium_transmittance(float sigmaT, float len) { return expf(-(sigmaT * len)); }

// the Halton index of the sample the lane is tracing: launch_device.hpp, which holds the words it is made of
DMT_DEV uint32_t medium_h(KArgs k, PathState const& st);
DMT_DEV MediumParams load_medium(KArgs k) {
  k = kargs(k);
  MediumParams m;
  m.sigmaT = k->medium.sigmaT, m.g = k->medium.g;
#pragma unroll
  for (int i = 0; i < 3; ++i) m.albedo[i] = k->medium.albedo[i], m.lo[i] = k->medium.lo[i], m.hi[i] = k->medium.hi[i];
  return m;
}
// the part of the segment o + t d, 0 <= t <= tEnd, inside the box, and its length
DMT_DEV bool medium_box_segment(MediumParams const& m, f3 o, f3 d, float tEnd, float* t0, float* t1) {
  float const o3[3] = {o.x, o.y, o.z}, d3[3] = {d.x, d.y, d.z};
  return medium_segment(o3, d3, tEnd, m.lo, m.hi, t0, t1);
}
DMT_DEV float medium_length(MediumParams const& m, f3 o, f3 d, float tEnd) {
  float t0, t1;
  return medium_box_segment(m, o, d, tEnd, &t0, &t1) ? t1 - t0 : 0.f;
}
// the grid as the kernel arguments hold it, and the march of the segment o + t d, 0 <= t <= tEnd, up to tauTarget
DMT_DEV MediumGridParams load_medium_grid(KArgs k) {
  k = kargs(k);
  MediumGridParams g;
  g.density = k->mediumGrid.density;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g.n[i] = k->mediumGrid.n[i], g.cell[i] = k->mediumGrid.cell[i], g.invCell[i] = k->mediumGrid.invCell[i];
    g.imin[i] = k->mediumGrid.imin[i], g.imax[i] = k->mediumGrid.imax[i], g.slo[i] = k->mediumGrid.slo[i], g.shi[i] = k->mediumGrid.shi[i];
  }
  return g;
}
DMT_DEV MediumGridMarch medium_grid_walk(KArgs k, MediumParams const& m, f3 o, f3 d, float tEnd, float tauTarget) {
  MediumGridParams const g = load_medium_grid(k);
  float const o3[3] = {o.x, o.y, o.z}, d3[3] = {d.x, d.y, d.z};
  return medium_grid_march(o3, d3, tEnd, tauTarget, m.sigmaT, m.lo, m.hi, g);
}
// the optical depth of the whole segment: the march's under a grid, sigmaT times the length inside the box without one
template <uint32_t F>
DMT_DEV float medium_segment_tau(KArgs k, MediumParams const& m, f3 o, f3 d, float tEnd) {
  if constexpr (F & kFeatMediumGrid) return medium_grid_walk(k, m, o, d, tEnd, kInf).tau;
  else return m.sigmaT * medium_length(m, o, d, tEnd);
}
DMT_DEV MediumSpectrumParams load_medium_spectrum(KArgs k) {
  k = kargs(k);
  MediumSpectrumParams s;
#pragma unroll
  for (int i = 0; i < 3; ++i) s.q[i] = k->mediumSpectrum.q[i], s.le[i] = k->mediumSpectrum.le[i];
  return s;
}
// exp(-q_c tau) per channel; a channel with q_c == 0 passes untouched
DMT_DEV f3 medium_spectrum_transmittance(MediumSpectrumParams const& s, float tau) {
  return mk3(s.q[0] > 0.f ? expf(-(s.q[0] * tau)) : 1.f, s.q[1] > 0.f ? expf(-(s.q[1] * tau)) : 1.f, s.q[2] > 0.f ? expf(-(s.q[2] * tau)) : 1.f);
}
// The NEE contribution the shading step has just left pending (st.hasShadow), times the transmittance of its shadow
// segment: every pending contribution of a medium row, made at a surface or at a scatter vertex, passes through here.
// The *_rgb rows take the segment's optical depth in the reference channel once, then the factor per channel.  The grey
// rows keep the skip tests they have had: the closed form asks the length, which can be > 0 where sigmaT times it is not.
template <uint32_t F>
DMT_DEV void medium_attenuate_pending(KArgs k, PathState const& st) {
  MediumParams const m = load_medium(k);
  f3 const o = shadow_org(st), d = shadow_dir(st);
  if constexpr (F & (kFeatMediumGrid | kFeatMediumSpectrum)) {
    float const tau = medium_segment_tau<F>(k, m, o, d, st.smax);
    if constexpr (F & kFeatMediumSpectrum) {
      if (tau > 0.f) put_C(get_C() * medium_spectrum_transmittance(load_medium_spectrum(k), tau));
    } else {
      if (tau != 0.f) put_C(get_C() * expf(-tau));
    }
  } else {
    float const len = medium_length(m, o, d, st.smax);
    if (len > 0.f) put_C(get_C() * medium_transmittance(m.sigmaT, len));
  }
}

enum : int { MV_THROUGH = 0, MV_ENDED = 1, MV_SCATTERED = 2 };
// The path segment that has just been traced (st's ray, ending at the hit bestTri or nowhere) against the medium.
// MV_THROUGH: no collision, path_shade goes on to the surface or the miss with st untouched (st.rng included); in the
// *_rgb rows st.beta carries the pass weights.
// MV_SCATTERED: the path scattered inside the box; NEE and the bounce are done, st holds the next ray.  MV_ENDED: the path
// ends at the scatter vertex (bounce cap, all-zero albedo, roulette).
template <uint32_t F>
DMT_DEV int medium_vertex(KArgs k, PathState& st, SceneView const& sc, int bestTri, float bu, float bv) {
  MediumParams const m = load_medium(k);
  f3 const o = ray_org(st), d = ray_dir(st);
  float tHit = kInf;
  if (bestTri >= 0) tHit = dot(shade_hit<F>(k, sc, bestTri, bu, bv, d).pos - o, d);
  float tColl;
  if constexpr (F & kFeatMediumSpectrum) {
    MediumSpectrumParams const sp = load_medium_spectrum(k);
    float const beta3[3] = {st.beta.x, st.beta.y, st.beta.z};
    uint32_t const h = medium_h(k, st);
    MediumSpectrumEvent ev;
    if constexpr (F & kFeatMediumGrid) {  // the march decides: it collides where the channel-m optical depth reaches T
      MediumSpectrumChoice const ch = medium_spectrum_choose(sp.q, beta3, h, uint32_t(st.depth));
      MediumGridMarch const r = medium_grid_walk(k, m, o, d, tHit, ch.T);
      if (!r.collided && !(r.tau > 0.f)) return MV_THROUGH;
      ev = medium_spectrum_weights(sp.q, ch, r.collided != 0, r.collided ? ch.T : r.tau);
      tColl = r.ts;
    } else {
      float t0, t1;
      if (!medium_box_segment(m, o, d, tHit, &t0, &t1)) return MV_THROUGH;
      float const tauSeg = m.sigmaT * (t1 - t0);
      if (!(tauSeg > 0.f)) return MV_THROUGH;
      ev = medium_spectrum_event(sp.q, beta3, h, uint32_t(st.depth), tauSeg);
      tColl = fminf(t0 + ev.tauAt / m.sigmaT, t1);
    }
    f3 const w = mk3(ev.w[0], ev.w[1], ev.w[2]);
    if (!ev.collided) {
      st.beta = st.beta * w;
      return MV_THROUGH;
    }
    // emission at the collision, before the depth cap, as a surface adds its own before it; then the weights
    st.L = st.L + st.beta * w * (mk3(1.f - m.albedo[0], 1.f - m.albedo[1], 1.f - m.albedo[2]) * mk3(sp.le[0], sp.le[1], sp.le[2]));
    st.beta = st.beta * w;
  } else if constexpr (F & kFeatMediumGrid) {  // the collision is where the optical depth along the segment reaches -log1p(-u)
    MediumGridMarch const r = medium_grid_walk(k, m, o, d, tHit, -log1pf(-medium_u(medium_h(k, st), uint32_t(st.depth))));
    if (!r.collided) return MV_THROUGH;
    tColl = r.ts;
  } else {
    float t0, t1;
    if (!medium_box_segment(m, o, d, tHit, &t0, &t1)) return MV_THROUGH;
    float const s = medium_free_flight(m.sigmaT, medium_u(medium_h(k, st), uint32_t(st.depth)));
    if (!(t0 + s < t1)) return MV_THROUGH;  // through with probability = the transmittance: beta stays as it is
    tColl = t0 + s;
  }
  f3 const p = o + tColl * d;
  if (st.depth >= kargs(k)->maxDepth) return MV_ENDED;
  f3 const albedo = mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
  if (is_zero(albedo)) return MV_ENDED;
  f3 const wo = -d;

  // next-event estimation: the draws and the light choice of a surface bounce, the phase function for the material
  float uLight = st.rng.get1D();
  f2 const uLight2 = st.rng.get2D();
  bool envNee = false;
  if constexpr (F & kFeatEnv) {
    envNee = uLight < 0.5f;
    uLight = envNee ? uLight : (uLight - 0.5f) * 2.f;
    if (envNee) {
      EnvView const env = load_env(k);
      EnvSampleDev const es = env_sample(env, uLight2);
      if (es.ok) {
        float const ph = hg_eval(m.g, dot(wo, es.wi));
        f3 const f = albedo * ph;
        f3 const Le = env_eval_uv(env, es.uv);
        if (!is_zero(f) && max3(Le) > 0.f) {
          put_C(st.beta * (Le * f / (es.pdf * 0.5f + ph)));
          set_shadow_ray(st, p, es.wi);
          st.smax = kInf;
          st.hasShadow = true;
        }
      }
    }
  }
  if (!envNee && sc.lightCount > 0) {
    uint32_t const li = pick_index(uLight, sc.lightCount);
    float const pmf = ((F & kFeatEnv) ? 0.5f : 1.f) / float(sc.lightCount);
    Rec32 const light = sc.lights[li];
    LightSample const ls = sample_light(light, p, uLight2, true, wo);  // hadT: no surface normal is asked of a point in space
    if (ls.valid()) {
      float const ph = hg_eval(m.g, dot(wo, ls.direction));
      f3 const f = albedo * ph;
      if (!is_zero(f)) {
        f3 const Le = eval_light(light, ls);
        if (ls.delta) {
          put_C(st.beta * Le * f / pmf);
        } else {
          float const w = sqr(pmf * ls.pdf) / sqr(pmf * ls.pdf + ph);
          put_C(Le * f * st.beta * w);
        }
        set_shadow_ray(st, p, ls.direction);
        st.smax = ls.distance;
        st.hasShadow = true;
      }
    }
  }
  if (st.hasShadow) medium_attenuate_pending<F>(k, st);

  // bounce: get2D + get1D as at a surface (the last value unused); f / pdf == 1
  f2 const u2 = st.rng.get2D();
  (void)st.rng.get1D();
  float const wo3[3] = {wo.x, wo.y, wo.z};
  float wi3[3], pdf;
  hg_sample(m.g, wo3, u2.x, u2.y, wi3, &pdf);
  st.lastT = false;
  st.lastPdf = pdf, st.lastSpecular = false;
  set_ray(st, p, mk3(wi3[0], wi3[1], wi3[2]));
  st.beta = st.beta * albedo;
  float const rrBeta = max3(st.beta);
  if (rrBeta < 1 && st.depth > 1) {
    float const q = fmaxf(0.f, 1.f - rrBeta);
    if (st.rng.get1D() < q) return MV_ENDED;
    st.beta = st.beta / (1 - q);
  }
  ++st.depth;
  return MV_SCATTERED;
}
