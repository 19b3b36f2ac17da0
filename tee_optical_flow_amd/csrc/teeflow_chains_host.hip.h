// Several chains of one frame size in lock-step, step k solving pair k of every chain still running as one batch: tf_calc_chains, _device, _rgb and their checks.
// Relies on teeflow_queue.hip.h (start_call, queue_finish, ChainSet) and, for the RGB form, on condition_to_device of teeflow_frames_host.hip.h.

namespace {
// The arguments of a lock-step call -> its chains in the library's order and the Call that carries them, or the refusal; before any GPU
// work.  frames / flows_out: one pointer per chain, in the caller's order, where `where` says.  armed: the three flags, which the call has spent.
int check_chains(tf_handle* h, const void* const* frames, const int* n_frames, int n_chains, int H, int W, float scale, void* const* flows_out,
                 int where, bool out_f16, const tf_handle::Armed& armed, ChainSet* cs, Call* c)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (armed.frames) return fail(h, TF_ERR_UNSUPPORTED, "tf_frames_next was armed: chains in lock-step take their frames from the caller's pointers (the flag is spent)");
    if (armed.hold) return fail(h, TF_ERR_UNSUPPORTED, "tf_hold_next was armed: chains in lock-step hold nothing (the flag is spent; a study call holds a study)");
    if (n_chains < 1) return fail(h, TF_ERR_INVALID_ARG, "chains in lock-step: n_chains must be >= 1, got %d", n_chains);
    if (!frames || !n_frames || !flows_out) return fail(h, TF_ERR_INVALID_ARG, "chains in lock-step: null frames, n_frames or flows_out array");
    for (int i = 0; i < n_chains; ++i) {
        if (!frames[i] || !flows_out[i]) return fail(h, TF_ERR_INVALID_ARG, "chains in lock-step: null frame or flow pointer of chain %d", i);
        if (n_frames[i] < 2) return fail(h, TF_ERR_INVALID_ARG, "chain %d has %d frames: a chain needs at least 2 frames", i, n_frames[i]);
    }
    if (h->P.algo == TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_UNSUPPORTED, "chains in lock-step are DualTVL1's (useInitialFlow): DeepFlow takes no initial flow");
    if (h->P.variant == TF_VARIANT_CUDA) return fail(h, TF_ERR_UNSUPPORTED, "chains in lock-step need useInitialFlow, which TF_VARIANT_CUDA does not implement");
    if (!h->P.use_initial_flow)
        return fail(h, TF_ERR_UNSUPPORTED, "useInitialFlow is clear: cv2 then ignores a passed flow, so the chains would be plain solves; set "
                                            "TF_PARAM_USE_INITIAL_FLOW first, or make the plain calls");
    const int limit = h->P.max_batch > 0 ? h->P.max_batch : DEFAULT_MAX_BATCH;
    if (n_chains > limit)
        return fail(h, TF_ERR_UNSUPPORTED, "%d chains in lock-step: a call takes at most %d, the pairs of one sub-batch (max_batch), since a step "
                                            "solves one pair of every chain together", n_chains, limit);
    long long total = 0;
    std::vector<size_t> first(n_chains);
    for (int i = 0; i < n_chains; ++i) { first[i] = (size_t)total; total += n_frames[i] - 1; }
    if (total > std::numeric_limits<int>::max()) return fail(h, TF_ERR_INVALID_ARG, "chains in lock-step: %lld pairs in one call", total);
    cs->order = chain_order(n_frames, n_chains);
    for (int i : cs->order) {
        cs->in.push_back((const uint8_t*)frames[i]); cs->out.push_back(flows_out[i]);
        cs->pairs.push_back(n_frames[i] - 1); cs->first.push_back(first[i]);
    }
    *c = Call{MODE_SEQ, cs->in[0], nullptr, (int)total, H, W, scale, cs->out[0], where, false, out_f16};
    c->chain = true; c->chains = cs;
    return check_call(h, *c);
}

// a checked lock-step call, solved and waited for: tf_get_iters then gives the counts chain after chain in the caller's order
int run_chains(tf_handle* h, const Call& c, tf_stats* st)
{
    QJob j;
    start_call(h, c, &j, false);
    return queue_finish(h, &j, st);
}

int chains_entry(tf_handle* h, const void* const* frames, const int* n_frames, int n_chains, int H, int W, float scale, void* const* flows_out,
                 int where, tf_stats* st)
{
    ChainSet cs; Call c;
    const int rc = check_chains(h, frames, n_frames, n_chains, H, W, scale, flows_out, where, false, spend(h, SPEND_ALL), &cs, &c);
    return rc ? rc : run_chains(h, c, st);
}
}  // namespace

TF_API int tf_calc_chains(tf_handle* h, const uint8_t* const* frames, const int* n_frames, int n_chains, int H, int W, float scale,
                          float* const* flows_out, tf_stats* st)
{
    return chains_entry(h, (const void* const*)frames, n_frames, n_chains, H, W, scale, (void* const*)flows_out, W_HOST, st);
}
TF_API int tf_calc_chains_device(tf_handle* h, const uint8_t* const* dframes, const int* n_frames, int n_chains, int H, int W, float scale,
                                 float* const* dflows_out, tf_stats* st)
{
    return chains_entry(h, (const void* const*)dframes, n_frames, n_chains, H, W, scale, (void* const*)dflows_out, W_DEV, st);
}

// the library's order of the chains of a lock-step call (pure host arithmetic, no device call): order_out[s] = the caller's index of the
// chain in state slot s; first_pair_out[i] = where chain i's pairs start in tf_get_iters' output
TF_API int tf_dbg_chain_order(const int* n_frames, int n_chains, int* order_out, long long* first_pair_out)
{
    if (!n_frames || n_chains < 1 || !order_out) return TF_ERR_INVALID_ARG;
    const std::vector<int> order = chain_order(n_frames, n_chains);
    long long total = 0;
    for (int i = 0; i < n_chains; ++i) {
        order_out[i] = order[i];
        if (first_pair_out) first_pair_out[i] = total;
        total += n_frames[i] - 1;
    }
    return TF_OK;
}

// Several RGB studies of one frame size as chains in lock-step: each study is conditioned as tf_calc_seq_rgb
// conditions it, one after the other into one scratch slot that holds all their gray frames; its echo, where asked for, comes from the same
// upload.  The flags are spent first, the arguments checked on the host pointers before anything is uploaded.
TF_API int tf_calc_chains_rgb(tf_handle* h, const uint8_t* const* rgb, const int* n_frames, int n_chains, int H, int W, float scale, int out_f16,
                              void* const* flows_out, uint16_t* const* echo16_out, tf_stats* st)
{
    const tf_handle::Armed armed = spend(h, SPEND_ALL);
    auto run = [&]() -> int {
        ChainSet cs; Call c;
        int rc = check_chains(h, (const void* const*)rgb, n_frames, n_chains, H, W, scale, flows_out, W_HOST, out_f16 != 0, armed, &cs, &c);
        if (rc) return rc;
        HIPC(h, hipSetDevice(h->dev));                        // (the scratch below is this handle's device's, whatever the thread's current one)
        const size_t npx = (size_t)H * W;
        Pre pre(h);
        uint8_t* at = pre.get<uint8_t>(tf_handle::PRE_CH_GRAY, ((size_t)c.n_pairs + (size_t)n_chains) * npx);
        if (pre.rc) return pre.rc;
        for (int s = 0; s < cs.count(); ++s) {
            const int N = cs.pairs[s] + 1;
            const uint8_t* dgray = nullptr;
            rc = condition_to_device(h, Src::on_host(cs.in[s]), N, H, W, &dgray, at, echo16_out ? echo16_out[cs.order[s]] : nullptr);
            if (rc) return rc;
            cs.in[s] = dgray; at += (size_t)N * npx;
        }
        c.in0 = cs.in[0]; c.where = W_IN_DEV;
        return run_chains(h, c, st);
    };
    return finish_host_call(h, run());
}
