// The traversal loop of rt_persistent_kernel (rt_kernels.hip), included there inside the kernel's body: once in place with OCC false, and,
// in the kernels that hold the occlusion-only form (OCC_LOOP), inside a generic lambda that is instantiated for OCC false and true.
// Everything it names -- the lane's ray state, the stack helpers, OCC, occ -- is the including scope's.
    for (;;) {
      RT_LOOP_MARK("loop_top");
      if (!is_trace_job(JOB) && !EXACT) ++lpt_work;   // (wave-uniform: one scalar add per iteration)
      if (STATS && A.wave_log) {
        const unsigned long long nm = __ballot(is_node_desc(cur));
        ++wl_iter;
        if (nm) {
          ++wl_node_x; wl_node_l += (unsigned)__popcll(nm);
          const uint32_t c0 = __shfl(cur, __ffsll((long long)nm) - 1);
          if (__ballot(is_node_desc(cur) && cur == c0) == nm) ++wl_no3;   // every node lane of the wavefront is at the same node
        }
      }
      if (STATS && A.wave_log) wl_t0 = __builtin_readcyclecounter();
      unsigned wl_tag = 0;   // wave log: 1 + class + 4 * arm of this iteration's node-body run, in the lanes that took it
      if constexpr (PHASE_COUNT) {   // (counting variant: this iteration's node-body run by the form of the loop and the rays its wavefront holds)
        if (__any(is_node_desc(cur))) {
          if (OCC) ++ph_cnt[3];
          else if (__any(is_work_desc(cur) && (flags & F_ANYHIT) != 0u)) ++ph_cnt[5];
          else ++ph_cnt[4];
        }
      }
      RT_LOOP_MARK("node");
      if (is_node_desc(cur)) {
        // ---- internal node: 4 box tests, order, push the far ones, continue with the nearest ----
        const bool top = !IDENT && (cur >> 30) == DK_TLAS;   // (IDENT: no lane is at TLAS level inside the loop)
        if (top && !(flags & F_WORLD)) {   // back at TLAS level after an instance (multi-instance scenes only)
          float ox, oy, oz, dx, dy, dz, tm;
          world_ray(ox, oy, oz, dx, dy, dz, tm);
          arx = ox; ary = oy; arz = oz; aix = 1.0f / dx; aiy = 1.0f / dy; aiz = 1.0f / dz;
          flags |= F_WORLD;
        }
        const uint32_t ni = cur & PAYLOAD_MASK;
        uint4 q0, q1, q2, q3;
        if (USE_TOP && (cur & DESC_TOP_FLAG)) {
          // (volatile, LDS-typed pointer: through plain pointers the compiler merges the two arms into FLAT loads of a
          // selected address -- thirteen flat_load instead of four ds_read_b128 / global_load_dwordx4)
          typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
          typedef __attribute__((address_space(3))) const volatile u32x4_t lds_u32x4_t;
          lds_u32x4_t* tp = (lds_u32x4_t*)&s_top[0][0] + (cur & DESC_TOP_SLOT);
          const u32x4_t t0 = tp[0], t1 = tp[RT_TOP_NODES], t2 = tp[2 * RT_TOP_NODES], t3 = tp[3 * RT_TOP_NODES];
          q0 = make_uint4(t0.x, t0.y, t0.z, t0.w); q1 = make_uint4(t1.x, t1.y, t1.z, t1.w);
          q2 = make_uint4(t2.x, t2.y, t2.z, t2.w); q3 = make_uint4(t3.x, t3.y, t3.z, t3.w);
          if (STATS && A.wave_log) ++wl_no23;
        } else {
          const uint4* np = sc.nodes_c + (size_t)ni * CNODE_VEC4;
          q0 = np[0]; q1 = np[1]; q2 = np[2]; q3 = np[3];
        }
        const uint32_t* ref_node = nullptr;
        if (LDEXP) ref_node = top ? sc.ref_tlas + (size_t)ni * RT_NODE_DWORDS : sc.ref_bvh + (size_t)(ni - sc.n_tlas) * RT_NODE_DWORDS;
        if (STATS) fx.node++;
        Cand c[4];
        // timed plain / shadow frame jobs: the occlusion arm works on the box tests' own masks (RT_OCC_OK_MASKS)
        constexpr bool OK_MASKS = RT_OCC_OK_MASKS && !EXACT && STATS == 0 && !ALPHA && (job_base(JOB) == JOB_RENDER || job_base(JOB) == JOB_RENDER_SHADOW);
        bool ok[4] = {false, false, false, false};
        if (OK_MASKS) eval_children_raw<EXACT, LDEXP, BOX_NO_SELECT>(q0, q1, q2, q3, ref_node, arx, ary, arz, aix, aiy, aiz, hitd, c, ok);
        else eval_children<EXACT, LDEXP>(q0, q1, q2, q3, ref_node, arx, ary, arz, aix, aiy, aiz, hitd, c);
        // wave log of the timed traversal's counting build (STATS == 2 only): this run's class = the largest number of valid children any of
        // its node lanes holds (0, 1, 2, >= 3); the arm adds 4 for the occlusion arm, and the run is counted behind the node body, where every
        // lane of the wavefront is active again.  The clocks the classing takes are taken out of the node body's window (wl_t0 moves on).
        if (STATS == 2 && A.wave_log) {
          const unsigned long long ta = __builtin_readcyclecounter();
          const bool v[4] = {c[0].d < __builtin_inff(), c[1].d < __builtin_inff(), c[2].d < __builtin_inff(), c[3].d < __builtin_inff()};
          wl_tag = 1u + (__any(order_three_valid(v)) ? 3u : (__any(order_two_valid(v)) ? 2u : (__any(order_any_valid(v)) ? 1u : 0u)));
          wl_t0 += __builtin_readcyclecounter() - ta;
        }
        RT_LOOP_MARK("stack");
        // (the occlusion-only loop has the answer from its entry: no ballot per step, no ordered arm)
        if (OCC || (((job_base(JOB) == JOB_RENDER_SHADOW && RT_UNORDERED_OCCLUSION) || JOB == JOB_TRACE_UNORDERED) && STATS != 1 && __all((flags & F_ANYHIT) != 0u))) {   // STATS keeps the reference's order, hence its fetch counts
          // occlusion rays of a frame only feed a boolean (is anything hit before the light?): the set
          // of triangles an any-hit traversal can reach does not depend on the visiting order, so the
          // ordering network and the path_m bookkeeping are skipped (vxrt_trace's MODE_ANY, which
          // returns the reference's FIRST accepted candidate, keeps the ordered path)
          // (OK_MASKS: c[k].d is the raw slab distance here -- an occlusion ray's pushed distance is only ever compared with its constant hitd,
          // and a child that is pushed carries the same value in both forms)
          const bool v0 = OK_MASKS ? ok[0] : c[0].d < __builtin_inff(), v1 = OK_MASKS ? ok[1] : c[1].d < __builtin_inff();
          const bool v2 = OK_MASKS ? ok[2] : c[2].d < __builtin_inff(), v3 = OK_MASKS ? ok[3] : c[3].d < __builtin_inff();
          if (STATS == 2 && A.wave_log) wl_tag += 4u;
          if constexpr (OCC && HINTS) {
            // RT_SHADOW_HINTS (occlusion-only loop): the step below on the children in the order d0 .. d3 / w0 .. w3.  A run without a guided
            // lane (wave-uniform test) leaves them in slot order: today's step.  In a run with one, a guided lane whose hinted slot passed its
            // box test moves that child to the front -- the others keep their slot order behind it -- and shifts its code; a guided lane whose
            // hinted slot failed is guided no more.  All of it selects: no per-lane branch.
            uint32_t d0 = c[0].desc, d1 = c[1].desc, d2 = c[2].desc, d3 = c[3].desc;
            bool w0 = v0, w1 = v1, w2 = v2, w3 = v3;
            if (__any((flags & F_GUIDED) != 0u)) {
              const uint32_t code = __float_as_uint(path_m), hs = code & 3u;
              // (conditions as and / or of lane masks: written as selects they become per-lane branches)
              const bool g = (flags & F_GUIDED) != 0u && ((hs == 0u && v0) || (hs == 1u && v1) || (hs == 2u && v2) || (hs == 3u && v3));
              path_m = __uint_as_float(g ? code >> 2 : code);
              flags = g ? flags : (flags & ~F_GUIDED);
              const bool m1 = g && hs >= 1u, m2 = g && hs >= 2u, m3 = g && hs == 3u;   // slot 0 .. 2 moves one place back
              const uint32_t dh = hs == 1u ? d1 : (hs == 2u ? d2 : d3);
              d3 = m3 ? d2 : d3; d2 = m2 ? d1 : d2; d1 = m1 ? d0 : d1; d0 = m1 ? dh : d0;
              w3 = (m3 && w2) || (!m3 && w3); w2 = (m2 && w1) || (!m2 && w2); w1 = (m1 && w0) || (!m1 && w1); w0 = m1 || w0;
            }
            if (w0 || w1 || w2 || w3) {
              bool more = true;
              if (sp + 4 > STACK_CAP) { atomicOr(A.status, STATUS_STACK_OVERFLOW); more = false; }
              cur = w0 ? d0 : (w1 ? d1 : (w2 ? d2 : d3));
              push_pending(occ, more && w1 && w0, d1, 0.f, more && w2 && (w0 || w1), d2, 0.f, more && w3 && (w0 || w1 || w2), d3, 0.f);   // (no path maximum in this loop's entries)
            } else {
              pop_next(occ);
            }
          } else
          if (v0 || v1 || v2 || v3) {
            bool more = true;
            if (sp + 4 > STACK_CAP) { atomicOr(A.status, STATUS_STACK_OVERFLOW); more = false; }
            cur = v0 ? c[0].desc : (v1 ? c[1].desc : (v2 ? c[2].desc : c[3].desc));
            // (slot order: the first valid child is visited, the others are pushed as they come)
            push_pending(occ, more && v1 && v0, c[1].desc, c[1].d, more && v2 && (v0 || v1), c[2].desc, c[2].d, more && v3 && (v0 || v1 || v2), c[3].desc, c[3].d);
          } else {
            pop_next(occ);
          }
        } else {
          // RT_ORDER_PATHS: a run none of whose lanes holds more than one valid child has nothing to sort and nothing to push.  The test is
          // wave-uniform, over the node lanes the phase ballot above ranged over; the conditions live in scalar masks.  The identity-root
          // shadow frame kernels only (see the knob in rt_kernels.hip).
          constexpr bool ORDER_PATHS = OK_MASKS && IDENT && job_base(JOB) == JOB_RENDER_SHADOW && RT_ORDER_PATHS != 0;
          bool ordered = false;   // (wave-uniform: the step was taken without the network)
          if (ORDER_PATHS) {
            if (!__any(order_two_valid(ok))) {
              ordered = true;
              const bool any1 = order_any_valid(ok);
              if (RT_ORDER_CHECK) {   // what the network decides: the child taken, nothing pushed, the new maximum
                Cand n[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll
                for (int k = 0; k < 4; ++k) n[k].d = ok[k] ? n[k].d : __builtin_inff();
                order_children(n);
                bool bad = any1 != (n[0].d < __builtin_inff()) || n[1].d < __builtin_inff() || n[2].d < __builtin_inff() || n[3].d < __builtin_inff();
                if (any1) bad = bad || order_first_valid(c, ok).desc != n[0].desc || __float_as_uint(vmax_nonan(path_m, order_first_valid(c, ok).d)) != __float_as_uint(vmax_nonan(path_m, n[0].d));
                if (bad) atomicOr(A.status, STATUS_ITER_LIMIT);
              }
              if (any1) {
                // (the overflow test stands in front of every step that holds a valid child, whether it pushes or not)
                if (sp + 4 > STACK_CAP) atomicOr(A.status, STATUS_STACK_OVERFLOW);
                const Cand only = order_first_valid(c, ok);
                cur = only.desc;
                path_m = vmax_nonan(path_m, only.d);
              } else {
                pop_next(occ);
              }
            }
          }
          if (!ordered) {
            if (OK_MASKS) {
#pragma unroll
              for (int k = 0; k < 4; ++k) c[k].d = ok[k] ? c[k].d : __builtin_inff();
            }
            order_children(c);   // valid children first (d < inf), nearest in c[0]
            // (path_m and the candidates' distances are never NaN -- a filtered child carries +inf -- so the maxima need no
            // canonicalising v_max x, x in front of them)
            if (c[0].d < __builtin_inff()) {
              bool more = true;
              if (sp + 4 > STACK_CAP) { atomicOr(A.status, STATUS_STACK_OVERFLOW); more = false; }
              // far first so that the nearest pending sibling is on top (:98-103)
              push_pending(occ, more && c[3].d < __builtin_inff(), c[3].desc, vmax_nonan(path_m, c[3].d), more && c[2].d < __builtin_inff(), c[2].desc, vmax_nonan(path_m, c[2].d),
                           more && c[1].d < __builtin_inff(), c[1].desc, vmax_nonan(path_m, c[1].d));
              cur = c[0].desc;
              path_m = vmax_nonan(path_m, c[0].d);
            } else {
              pop_next(occ);
            }
          }
        }
      }
      if (STATS && A.wave_log) { const unsigned long long t1 = __builtin_readcyclecounter(); wl_tn += t1 - wl_t0; wl_t0 = t1; }
      if (STATS == 2 && A.wave_log) {
        const unsigned long long tm = __ballot(wl_tag != 0u);
        if (tm) {
          const unsigned tag = __shfl(wl_tag, __ffsll((long long)tm) - 1) - 1u;   // (the same in every lane that took the run)
#pragma unroll
          for (unsigned k = 0; k < 8; ++k) wl_cc[k] += tag == k ? 1u : 0u;
        }
        wl_t0 = __builtin_readcyclecounter();   // (the count belongs to neither body's window)
      }
      RT_LOOP_MARK("inst");
      if (!IDENT && __any(is_inst_desc(cur))) {
        if (is_inst_desc(cur)) {
          float ox, oy, oz, dx, dy, dz, tm;
          world_ray(ox, oy, oz, dx, dy, dz, tm);
          enter_instance(cur & PAYLOAD_MASK, ox, oy, oz, dx, dy, dz);
        }
      }
      // leaves are postponed until RT_LEAF_MIN lanes hold one (or no lane has a node left): the leaf
      // body then runs for many lanes at once instead of once per iteration for a few
      RT_LOOP_MARK("leaf");
      const unsigned long long leafm = __ballot(is_leaf_desc(cur));
      if (leafm != 0ull && ((uint32_t)__popcll(leafm) >= (is_trace_job(JOB) ? RT_TRACE_LEAF_MIN : RT_LEAF_MIN) || __ballot(is_node_desc(cur) || (!IDENT && is_inst_desc(cur))) == 0ull)) {
        // ---- BLAS leaf (:123-161): triangles in index order, strict '<' ----
        if (STATS && A.wave_log) { ++wl_leaf_x; wl_leaf_l += (unsigned)__popcll(leafm); }
        if (!is_trace_job(JOB) && !EXACT) lpt_work += 2u;   // (a leaf-body run costs about 2.5 node-body runs: tools/wave_balance.py)
        {
          // triangles through LDS (RT_TRI_LDS): the lanes of a tile reach the same leaves, and every one of them loads the leaf's
          // triangles for itself.  The leaf of the first leaf lane is loaded ONCE, by 3 lanes per triangle, and handed to the lanes
          // that hold it by broadcast reads; the others load theirs as before.
          bool tri_from_lds = false;
          if (TRI_LDS) {
            const uint32_t L0 = __shfl(cur, __ffsll((long long)leafm) - 1);
            const uint32_t c0 = (L0 >> LEAF_FIRST_BITS) & LEAF_MAX_INLINE;
            const unsigned long long same = __ballot(cur == L0);
            if (c0 != 0u && c0 <= (uint32_t)RT_TRI_LDS && (uint32_t)__popcll(same) >= (uint32_t)RT_TRI_LDS_MIN) {   // (wave-uniform)
              if (lane < 3u * c0) s_tri[threadIdx.x >> 6][lane] = sc.tri_w[(size_t)(L0 & LEAF_FIRST_MASK) * 3 + lane];
              tri_from_lds = cur == L0;
              if (STATS && A.wave_log) wl_no23 += (unsigned)__popcll(same);
            }
          }
          if (is_leaf_desc(cur)) {
            if (STATS) fx.node++;
            uint32_t leftFirst = cur & LEAF_FIRST_MASK, triCount = (cur >> LEAF_FIRST_BITS) & LEAF_MAX_INLINE;
            if (triCount == 0u) {   // leaf with more than 15 triangles: range kept in the reference node
              const uint32_t* rn = sc.ref_bvh + (size_t)leftFirst * RT_NODE_DWORDS;
              leftFirst = rn[4]; triCount = rn[5];
            }
            const float cdx = __uint_as_float(CTX(0)), cdy = __uint_as_float(CTX(1)), cdz = __uint_as_float(CTX(2));
            bool stop = false;
            // ray buffers (incoherent rays, latency-bound leaves): the next triangle's 48 bytes are requested before the
            // current one is tested, +3 %; camera tiles lose 1.5 % to the extra registers, so they load in place
            constexpr bool PREFETCH = is_trace_job(JOB) && RT_TRI_PREFETCH;
            float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, n2 = n0;
            if (PREFETCH) { const float4* tp0 = sc.tri_w + (size_t)leftFirst * 3; n0 = tp0[0]; n1 = tp0[1]; n2 = tp0[2]; }
            // the plain / shadow frame jobs (RT_LEAF_FLAT above); the others keep the two-trip triangle test
            constexpr bool FLAT_TEST = RT_LEAF_FLAT >= 1 && !EXACT && !ALPHA && (job_base(JOB) == JOB_RENDER || job_base(JOB) == JOB_RENDER_SHADOW);
            RT_LOOP_MARK("leaf_tris");
            for (uint32_t i = 0; i < triCount; ++i) {
              const uint32_t triIdx = leftFirst + i;
              float4 t0, t1, t2;
              if (TRI_LDS && tri_from_lds) {
                // (typed LDS pointer: through a plain pointer the compiler would merge this arm and the global one into flat loads)
                typedef float f32x4_t __attribute__((ext_vector_type(4)));
                typedef __attribute__((address_space(3))) const volatile f32x4_t lds_f32x4_t;
                lds_f32x4_t* lp = (lds_f32x4_t*)&s_tri[threadIdx.x >> 6][0] + 3u * i;
                const f32x4_t a0 = lp[0], a1 = lp[1], a2 = lp[2];
                t0 = make_float4(a0.x, a0.y, a0.z, a0.w); t1 = make_float4(a1.x, a1.y, a1.z, a1.w); t2 = make_float4(a2.x, a2.y, a2.z, a2.w);
              } else
              if (PREFETCH) {
                t0 = n0; t1 = n1; t2 = n2;
                if (i + 1u < triCount) { const float4* tn = sc.tri_w + (size_t)(triIdx + 1u) * 3; n0 = tn[0]; n1 = tn[1]; n2 = tn[2]; }
              } else {
                const float4* tp = sc.tri_w + (size_t)triIdx * 3;
                t0 = tp[0]; t1 = tp[1]; t2 = tp[2];
              }
              if (STATS) fx.tri++;
              float bx, by, bz;
              const float d = FLAT_TEST ? ray_tri_flat(arx, ary, arz, cdx, cdy, cdz, t0, t1, t2, bx, by, bz) : ray_tri(arx, ary, arz, cdx, cdy, cdz, t0, t1, t2, bx, by, bz);
              if constexpr (OCC) {
                // an occlusion ray's accepted candidate ends it: the ray only feeds "is anything hit before the light" (no record: slots
                // 3-7 keep the pixel's primary hit; no flag tests; hitd is not read again once the ray has stopped)
                if constexpr (HINTS) { if (d < hitd) { flags |= F_FOUND | F_HINTW; path_m = __uint_as_float(triIdx); stop = true; break; } }   // (the blocker, for the finish section)
                else if (d < hitd) { flags |= F_FOUND; stop = true; break; }
              } else
              if (d < hitd) {
                // a rejected candidate is a triangle the ray missed: no record, no abandon test, no stop, on to the leaf's next triangle
                if constexpr (ALPHA) { if (alpha_rejects(sc, A.alpha_tri, triIdx, bx, by, bz)) continue; }
                hitd = d;
                flags |= F_FOUND;
                // (a frame's occlusion ray only feeds a boolean; slots 3-7 keep the pixel's primary hit meanwhile)
                if (!(job_base(JOB) == JOB_RENDER_SHADOW && (flags & F_SHADOW))) { CTX(3) = __float_as_uint(bx); CTX(4) = __float_as_uint(by); CTX(6) = CTX(8); CTX(7) = triIdx; }
                if (flags & F_ANYHIT) { stop = true; break; }
                // the reference re-descends from the root with the shrunken hit.dist; if any box on the
                // current path no longer passes `d < hit.dist` it abandons this subtree (DESIGN.md s3)
                if (!(path_m < hitd)) break;
              }
            }
            RT_LOOP_MARK("leaf_pop");
            if (stop) { sp = 0; tos_d = DESC_DONE; cur = DESC_DONE; }
            else pop_next(occ);
          }
        }
      }
      if (STATS && A.wave_log) { const unsigned long long t1 = __builtin_readcyclecounter(); wl_tl += t1 - wl_t0; }
      RT_LOOP_MARK("loop_exit");
      // leave when nothing traverses any more, or when enough lanes are dead weight AND leaving can
      // revive them (finished rays to retire, or idle lanes while jobs remain)
      const unsigned long long work = __ballot(is_work_desc(cur));
      if (work == 0ull) break;
      // (every lane that holds no work is finished or idle: while those are fewer than the smaller of the two bounds, neither test below
      // can hold, and the one ballot above has decided)
      if (RT_BATCH_PUSH && 64u - (uint32_t)__popcll(work) < (DEAD_MAX < FINISH_MIN ? DEAD_MAX : FINISH_MIN)) continue;
      const unsigned long long done = __ballot(cur == DESC_DONE);
      const uint32_t n_done = (uint32_t)__popcll(done);
      const uint32_t n_idle = queue_empty && loc_next == loc_end ? 0u : 64u - (uint32_t)__popcll(work | done);
      if (n_done + n_idle >= DEAD_MAX || n_done >= FINISH_MIN) break;
    }
