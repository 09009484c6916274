// The statements of the sampler's final workgroup for ONE row, kept as text: included once into each of its two entries in k_sample.hip (sample_final_kernel,
// sample_final_rows_kernel), which supply the names it reads -- cand, flags, nwg, pen, n (the row's candidate lists, NaN flags, slice count, penalised row, length),
// d (the row's ps_sample_dev), token_out (where the drawn id goes, may be null) and st / tokens / ids (the single-sequence step's bookkeeping; st == nullptr: none),
// and ENTRY (the entry's own instance of bitonic_sort_asc).
// As a __forceinline__ function the same statements compiled differently in sample_final_kernel (tools/isa_diff.py; HISTORY round 19 has the counts and the A/B);
// as text both entries get what the one kernel always got.  Not a stand-alone header: no include guard, no declarations of its own.
    __shared__ uint32_t smt[PS_MT_N];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sk[PS_SAMPLE_K_MAX];
    __shared__ ps_pi heap[PS_SAMPLE_K_MAX];
    __shared__ float tv[PS_SAMPLE_K_MAX];
    __shared__ int32_t tt[PS_SAMPLE_K_MAX];
    __shared__ double cp[PS_SAMPLE_K_MAX];
    __shared__ int surv[EX_CHUNK];
    __shared__ unsigned wsum[FN_NT / 64];
    __shared__ uint32_t sdk[DK_CAP];
    __shared__ double s_sum;
    __shared__ int s_nan, s_tie, s_r, s_eq, s_cnt, s_total, s_n, s_cut, s_idx;
    __shared__ uint32_t s_prefix, s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = d->k, kp1 = k + 1, n_cand = nwg * kp1;
    for (int i = tid; i < PS_MT_N; i += FN_NT) smt[i] = d->mt[i];
    if (tid == 0) { s_nan = 0; s_tie = 0; s_cnt = 0; s_next = 0xffffffffu; }
    __syncthreads();
    for (int i = tid; i < nwg; i += FN_NT)
        if (flags[i]) s_nan = 1;
    __syncthreads();
    bool exact = s_nan != 0;
    if (!exact) {
        // ---- fast path: the k-th smallest key (= k-th largest value), radix select 8 bits at a time
        // the high halves (value keys) in LDS when they fit; each thread walks a contiguous range (runs of one sorted slice list share
        // their digits: one LDS atomic per run instead of one per key)
        const bool staged = n_cand <= DK_CAP;
        if (staged) {
            int i = tid;
            for (; i + 3 * FN_NT < n_cand; i += 4 * FN_NT) {
                const unsigned long long a0 = cand[i], a1 = cand[i + FN_NT], a2 = cand[i + 2 * FN_NT], a3 = cand[i + 3 * FN_NT];
                sdk[i] = (uint32_t)(a0 >> 32); sdk[i + FN_NT] = (uint32_t)(a1 >> 32); sdk[i + 2 * FN_NT] = (uint32_t)(a2 >> 32); sdk[i + 3 * FN_NT] = (uint32_t)(a3 >> 32);
            }
            for (; i < n_cand; i += FN_NT) sdk[i] = (uint32_t)(cand[i] >> 32);
        }
        const int per = (n_cand + FN_NT - 1) / FN_NT, i0 = min(tid * per, n_cand), i1 = min(i0 + per, n_cand);
        uint32_t prefix = 0;
        int r = k;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += FN_NT) hist[i] = 0;
            __syncthreads();
            unsigned run_bin = 0xffffffffu, run_cnt = 0;
            for (int i = i0; i < i1; i++) {
                const uint32_t dk = staged ? sdk[i] : (uint32_t)(cand[i] >> 32);
                if (pass == 0 || (dk >> (shift + 8)) == prefix) {
                    const unsigned b = (dk >> shift) & 255;
                    if (b == run_bin) run_cnt++;
                    else { if (run_cnt) atomicAdd(&hist[run_bin], run_cnt); run_bin = b; run_cnt = 1; }
                }
            }
            if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
            __syncthreads();
            if (tid < 64) {
                unsigned h[4], s = 0;
                for (int j = 0; j < 4; j++) { h[j] = hist[4 * tid + j]; s += h[j]; }
                const unsigned incl = wave_incl_scan(s), excl = incl - s;
                if (excl < (unsigned)r && incl >= (unsigned)r) { // the bin that holds rank r
                    unsigned cum = excl;
                    for (int j = 0; j < 4; j++) {
                        if (cum + h[j] >= (unsigned)r) { s_r = r - (int)cum; s_prefix = (prefix << 8) | (uint32_t)(4 * tid + j); s_eq = (int)h[j]; break; }
                        cum += h[j];
                    }
                }
            }
            __syncthreads();
            r = s_r; prefix = s_prefix;
        }
        if (s_eq > r) exact = true; // the k-th and the (k+1)-th value have the same bits
        if (!exact) {
            uint32_t next = 0xffffffffu;
            for (int i = i0; i < i1; i++) {
                const uint32_t dk = staged ? sdk[i] : (uint32_t)(cand[i] >> 32);
                if (dk <= prefix) { const int slot = atomicAdd(&s_cnt, 1); if (slot < PS_SAMPLE_K_MAX) sk[slot] = cand[i]; }
                else next = min(next, dk);
            }
            atomicMin(&s_next, next);
            __syncthreads();
            for (int i = k + tid; i < PS_SAMPLE_K_MAX; i += FN_NT) sk[i] = ~0ull;
            bitonic_sort_asc<PS_SAMPLE_K_MAX, FN_NT, ENTRY>(sk);
            for (int i = tid; i < k; i += FN_NT) { // -0 and +0: different keys, equal values
                const float v = ckey_val(sk[i]), w = i + 1 < k ? ckey_val(sk[i + 1]) : fkey_val(~s_next);
                if (v == w) s_tie = 1;
                tv[i] = v; tt[i] = (int32_t)(uint32_t)sk[i];
            }
            __syncthreads();
            exact = s_tie != 0 || s_cnt != k;
        }
    }
    if (exact) {
        // ---- std::partial_sort's heap mechanics: make_heap over the first k entries, then every later entry that is greater than
        // the top replaces it.  Only an entry greater than the top at the start of its chunk can enter (the top only rises while no
        // NaN sits in the heap; when it falls, the rest of that chunk is walked entry by entry).
        if (tid == 0) {
            for (int i = 0; i < k; i++) heap[i] = ps_pi{pen[i], i};
            ps_make_heap(heap, k);
        }
        __syncthreads();
        for (int base = k; base < n; base += EX_CHUNK) {
            const float thr = heap[0].v;
            const int j0 = base + tid * EX_PER;
            unsigned m = 0;
#pragma unroll
            for (int e = 0; e < EX_PER; e++)
                if (j0 + e < n && pen[j0 + e] > thr) m |= 1u << e;
            const unsigned c = __popc(m), incl = wave_incl_scan(c);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            unsigned off = incl - c;
            for (int w = 0; w < wave; w++) off += wsum[w];
            for (int e = 0; e < EX_PER; e++)
                if (m & (1u << e)) surv[off++] = j0 + e;
            if (tid == FN_NT - 1) s_total = (int)off;
            __syncthreads();
            if (tid == 0) {
                const int end = min(base + EX_CHUNK, n);
                for (int s = 0; s < s_total; s++) {
                    const int i = surv[s];
                    const float v = pen[i];
                    if (!(v > heap[0].v)) continue;
                    ps_pop_heap_into(heap, k, ps_pi{v, i});
                    if (heap[0].v < thr) { // the top fell below the filter's threshold: the rest of the chunk one by one
                        for (int ii = i + 1; ii < end; ii++) {
                            const float vv = pen[ii];
                            if (vv > heap[0].v) ps_pop_heap_into(heap, k, ps_pi{vv, ii});
                        }
                        break;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            ps_sort_heap(heap, k);
            for (int i = 0; i < k; i++) { tv[i] = heap[i].v; tt[i] = heap[i].t; }
        }
    }
    __syncthreads();
    // ---- the chain's tail (ps_sample_tail, same operations): the per-candidate steps spread over the workgroup, the ordered sums and
    // the draw on thread 0
    const float temp = d->temperature, top_p = d->top_p;
    if (temp != 1)
        for (int i = tid; i < k; i += FN_NT) tv[i] /= temp;
    __syncthreads();
    const float top = tv[0];
    __syncthreads();
    for (int i = tid; i < k; i += FN_NT) tv[i] = ps_expf_glibc(tv[i] - top);
    __syncthreads();
    if (tid == 0) {
        double total = 0.;
        for (int i = k; i-- > 0;) total += tv[i];
        s_sum = total;
    }
    __syncthreads();
    for (int i = tid; i < k; i += FN_NT) tv[i] = (float)((double)tv[i] / s_sum);
    __syncthreads();
    if (tid == 0) {
        int n_keep = k, cut = 0;
        if (top_p < 1.0f) {
            float mass = 0.0f;
            int keep   = 0;
            while (keep < k) {
                mass += tv[keep++];
                if (mass >= top_p && keep >= 1) break;
            }
            if (keep < k) {
                n_keep = keep; cut = 1;
                double t2 = 0.;
                for (int i = 0; i < n_keep; i++) t2 += tv[i];
                s_sum = t2;
            }
        }
        s_n = n_keep; s_cut = cut;
    }
    __syncthreads();
    const int nk = s_n;
    if (s_cut)
        for (int i = tid; i < nk; i += FN_NT) tv[i] = (float)((double)tv[i] / s_sum);
    __syncthreads();
    uint64_t calls = 0;
    uint32_t p = d->mt_pos;
    if (nk >= 2) { // ps_discrete_draw
        if (tid == 0) {
            double sum = 0.0;
            for (int i = 0; i < nk; i++) sum += (double)tv[i];
            s_sum = sum;
        }
        __syncthreads();
        for (int i = tid; i < nk; i += FN_NT) cp[i] = (double)tv[i] / s_sum;
        __syncthreads();
        if (tid == 0) {
            double acc = cp[0];
            for (int i = 1; i < nk; i++) { acc = acc + cp[i]; cp[i] = acc; }
            cp[nk - 1] = 1.0;
            const double u = ps_mt_canonical(smt, &p);
            calls = 2;
            int first = 0, len = nk;
            while (len > 0) {
                const int half = len >> 1, mid = first + half;
                if (cp[mid] < u) { first = mid + 1; len = len - half - 1; }
                else len = half;
            }
            s_idx = first;
        }
    } else if (tid == 0) {
        s_idx = 0;
    }
    __syncthreads();
    if (tid == 0) {
        const int idx = s_idx;
        const int32_t tok = tt[idx];
        d->mt_pos = p;
        d->n_outputs += calls;
        d->n_exact += exact ? 1 : 0;
        if (token_out) token_out[0] = tok;
        if (st) { tokens[0] = tok; ids[st->n_out] = tok; st->n_out += 1; st->pos0 += 1; }
    }
    __syncthreads();
    for (int i = tid; i < PS_MT_N; i += FN_NT) d->mt[i] = smt[i];
