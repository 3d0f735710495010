// vox_batch_plan.cpp -- the batch planner: step costs, slot plan, slot schedule (no device)
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the device-free host units: DESIGN.md, "Host units")
#include "vox_host_base.h"

using namespace vox_host;

// Step costs the planner prices a session with: the table `base`, corrected by what the context has measured (`meas`, 0 = form not seen yet) -- a form seen before costs
// what it cost (clock, a shared GPU, another geometry), a form not seen yet the table's value times the mean measured / table ratio of the forms that were.  calib off
// (VOX_BATCH_NO_CALIB=1): the table alone.
namespace vox_host {
void step_costs(const double* base, const double* meas, bool calib, bool shared, double* out) {
    double ratio = 0.0; int nr = 0;
    for (int g2 = 1; g2 <= kMaxGroups; g2++) if (calib && meas[g2] > 0.0) { ratio += meas[g2] / base[g2]; nr++; }
    ratio = nr ? std::min(4.0, std::max(0.25, ratio / nr)) : 1.0;
    // The common factor (clock, a GPU shared with another session) is taken as measured; a form's deviation from it is trusted within +-15 % only, and a step of more
    // groups never costs less than one of fewer: next to a second session on the GPU (tools/two_sessions_probe.py) the per-form figures scatter (a 3-group step "measured"
    // at 5.35 ms against 4.18 for four groups made the next session plan 48 slots instead of 64: 4.71 s instead of 3.77 s for the corpus)
    out[0] = 0.0;
    for (int g2 = 1; g2 <= kMaxGroups; g2++) {
        const double common = base[g2] * ratio;
        out[g2] = (calib && !shared && meas[g2] > 0.0) ? common * std::min(1.15, std::max(0.85, meas[g2] / common)) : common;      // (a shared GPU: the common factor only)
        out[g2] = std::max(out[g2], out[g2 - 1]);
    }
}
}  // namespace vox_host
// jobs: (decode steps, utterance) with steps >= 1.  LPT onto 16 G slots, slots ordered by load (so the groups retire last to first), G by the cost model.
static SlotPlan plan_slots(const std::vector<std::pair<int, int>>& jobs_in, int force_G, const double* step_ms, int max_groups = 4) {
    std::vector<std::pair<int, int>> jobs = jobs_in;
    std::stable_sort(jobs.begin(), jobs.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first > b.first; });
    SlotPlan best;
    const int g_max = std::max(1, std::min(max_groups, ((int)jobs.size() + 15) / 16));
    for (int G = 1; G <= g_max; G++) {
        if (force_G > 0 && G != std::min(force_G, g_max)) continue;
        const int Sl = 16 * G;
        std::vector<long> load(Sl, 0); std::vector<std::vector<int>> q(Sl);
        for (auto& j : jobs) { int b = 0; for (int s2 = 1; s2 < Sl; s2++) if (load[s2] < load[b]) b = s2; load[b] += j.first; q[b].push_back(j.second); }
        std::vector<int> order(Sl); for (int i = 0; i < Sl; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return load[a] > load[b]; });
        SlotPlan pl; pl.G = G; pl.queue.resize(Sl); pl.steps_g.assign(G, 0);
        for (int i = 0; i < Sl; i++) { pl.queue[i] = q[order[i]]; pl.steps_g[i / 16] = std::max(pl.steps_g[i / 16], (int)load[order[i]]); }
        for (int k = 0; k < G; k++) pl.cost_ms += (double)(pl.steps_g[k] - (k + 1 < G ? pl.steps_g[k + 1] : 0)) * step_ms[k + 1];
        if (best.G == 0 || pl.cost_ms <= best.cost_ms) best = pl;
    }
    return best;
}
// SlotSchedule (vox_host_base.h): a plan as the decode loop uses it: the slot queues flattened (slot sl's k-th utterance at h_queue[sl q_stride + k], -1 behind its last), the steps of the whole
// decode, and how long each group RUNS.  A group retires when its queues are empty -- but every distinct set of active groups is a graph capture + instantiation
// (~10 ms): a group that would retire fewer than kRetireSlack steps before the next longer one keeps running with idle slots instead (harmless: idle rows compute on zeros).
static const int kRetireSlack = 12;
namespace vox_host {
SlotSchedule slot_schedule(const std::vector<std::pair<int, int>>& jobs, int force_G, const double* step_ms, int max_groups) {
    SlotSchedule z; z.plan = plan_slots(jobs, force_G, step_ms, max_groups);
    const SlotPlan& plan = z.plan;
    z.G = std::max(plan.G, 1); z.Sl = 16 * z.G;
    for (auto& q : plan.queue) z.q_stride = std::max(z.q_stride, (int)q.size() + 1);
    z.h_queue.assign((size_t)z.Sl * z.q_stride, -1);
    for (size_t sl = 0; sl < plan.queue.size(); sl++) for (size_t k = 0; k < plan.queue[sl].size(); k++) z.h_queue[sl * z.q_stride + k] = plan.queue[sl][k];
    z.steps = plan.steps_g.empty() ? 0 : plan.steps_g[0];
    for (size_t gi = 0; gi < plan.steps_g.size(); gi++) z.run_g[gi] = plan.steps_g[gi];
    for (int gi = 1; gi < z.G; gi++) {      // walk from the longest group down: snap a group to the previous one's run length when it is close
        if (z.run_g[gi - 1] - plan.steps_g[gi] < kRetireSlack) z.run_g[gi] = z.run_g[gi - 1];
    }
    return z;
}
}  // namespace vox_host
extern "C" int32_t vox_debug_step_costs(const double* base, const double* meas, int32_t calib, int32_t shared, double* out) {
    ARGCHK(base && meas && out, "null argument");
    step_costs(base, meas, calib != 0, shared != 0, out);
    return VOX_OK;
}
extern "C" int32_t vox_debug_plan_slots(const int32_t* steps, int32_t n, int32_t force_G, int32_t max_groups, const double* step_ms, int32_t* G, int32_t* job_slot,
                                        int32_t* job_qpos, int32_t* steps_g, int32_t* run_g, double* cost_ms) {
    ARGCHK(n >= 0 && (steps || n == 0) && step_ms && G && (job_slot || n == 0) && (job_qpos || n == 0) && steps_g && run_g && cost_ms, "null argument");
    ARGCHK(force_G >= 0 && force_G <= kMaxGroups && max_groups >= 1 && max_groups <= kMaxGroups, "group count out of range");
    std::vector<std::pair<int, int>> jobs;
    for (int i = 0; i < n; i++) { ARGCHK(steps[i] >= 1, "job %d: %d steps", i, steps[i]); jobs.emplace_back(steps[i], i); }
    const SlotSchedule z = slot_schedule(jobs, force_G, step_ms, max_groups);
    *G = z.G; *cost_ms = z.plan.cost_ms;
    for (int k = 0; k < kMaxGroups; k++) { steps_g[k] = k < (int)z.plan.steps_g.size() ? z.plan.steps_g[k] : 0; run_g[k] = z.run_g[k]; }
    for (int sl = 0; sl < z.Sl; sl++)
        for (int k = 0; k < z.q_stride; k++) { const int j = z.h_queue[(size_t)sl * z.q_stride + k]; if (j >= 0) { job_slot[j] = sl; job_qpos[j] = k; } }
    return VOX_OK;
}
