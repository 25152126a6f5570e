// Single pybind11 module for all ddls_amd HIP kernels.
#include <torch/extension.h>
#include <vector>

torch::Tensor row_mlp(torch::Tensor x, torch::Tensor ln_g, torch::Tensor ln_b,
                      torch::Tensor W, torch::Tensor b);
torch::Tensor message_reduce(torch::Tensor hn, torch::Tensor he,
                             torch::Tensor src, torch::Tensor edge_order,
                             torch::Tensor indptr, torch::Tensor ln_g,
                             torch::Tensor ln_b, torch::Tensor Wr,
                             torch::Tensor br);
torch::Tensor segment_mean(torch::Tensor x, torch::Tensor node_ptr, int64_t G);
std::vector<torch::Tensor> message_reduce_train(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src,
    torch::Tensor edge_order, torch::Tensor indptr, torch::Tensor ln_g,
    torch::Tensor ln_b, torch::Tensor Wr, torch::Tensor br);
std::vector<torch::Tensor> message_reduce_bwd(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src, torch::Tensor dst,
    torch::Tensor indptr, torch::Tensor ln_g, torch::Tensor ln_b,
    torch::Tensor Wr, torch::Tensor r_edge, torch::Tensor r_self,
    torch::Tensor gout);
std::vector<torch::Tensor> row_mlp_bwd(torch::Tensor x, torch::Tensor y,
                                       torch::Tensor gy, torch::Tensor ln_g,
                                       torch::Tensor ln_b, torch::Tensor W);
torch::Tensor row_mlp_mfma(torch::Tensor x, torch::Tensor ln_g,
                           torch::Tensor ln_b, torch::Tensor W,
                           torch::Tensor b);
std::vector<torch::Tensor> message_mlp_mfma(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src, torch::Tensor ln_g,
    torch::Tensor ln_b, torch::Tensor Wr, torch::Tensor br);
torch::Tensor segment_combine(torch::Tensor r_edge, torch::Tensor r_self,
                              torch::Tensor edge_order, torch::Tensor indptr);
torch::Tensor segment_mean_bwd(torch::Tensor gout, torch::Tensor node_ptr,
                               int64_t N);
std::vector<torch::Tensor> message_reduce_bwd_mfma(
    torch::Tensor hn, torch::Tensor he, torch::Tensor src, torch::Tensor dst,
    torch::Tensor indptr, torch::Tensor ln_g, torch::Tensor ln_b,
    torch::Tensor Wr, torch::Tensor r_edge, torch::Tensor r_self,
    torch::Tensor gout);
void flat_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, torch::Tensor step_t, torch::Tensor normsq,
               double clip, double lr, double b1, double b2, double eps);
void flat_sumsq(torch::Tensor x, torch::Tensor out);
void flat_sumsq_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                     torch::Tensor v, torch::Tensor step_t,
                     torch::Tensor normsq, torch::Tensor partials,
                     double clip, double lr, double b1, double b2,
                     double eps);
void flat_sumsq_adam_folded(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                            torch::Tensor v, torch::Tensor step_t,
                            torch::Tensor normsq, torch::Tensor partials,
                            torch::Tensor scratch, std::vector<int64_t> segs,
                            int64_t nsplit, int64_t stride, double clip,
                            double lr, double b1, double b2, double eps);
int64_t flat_sumsq_blocks(int64_t numel);
std::vector<torch::Tensor> head_fwd(
    torch::Tensor gm, torch::Tensor gf, torch::Tensor mask,
    torch::Tensor ln_w, torch::Tensor ln_b, torch::Tensor Wg,
    torch::Tensor bg, torch::Tensor W1p, torch::Tensor b1p,
    torch::Tensor W2p, torch::Tensor b2p, torch::Tensor W1v,
    torch::Tensor b1v, torch::Tensor W2v, torch::Tensor b2v);
std::vector<torch::Tensor> head_bwd(
    torch::Tensor gf, torch::Tensor emb, torch::Tensor h1p, torch::Tensor h1v,
    torch::Tensor glogits, torch::Tensor gvalue, torch::Tensor ln_w,
    torch::Tensor ln_b, torch::Tensor Wg, torch::Tensor W1p,
    torch::Tensor W2p, torch::Tensor W1v, torch::Tensor W2v);
std::vector<torch::Tensor> ppo_loss_fwd(
    torch::Tensor logits, torch::Tensor values, torch::Tensor actions,
    torch::Tensor old_logp, torch::Tensor adv, torch::Tensor vtarg,
    torch::Tensor kl_coef, double clip, double vf_clip, double vf_coef,
    double ent_coef);
std::vector<torch::Tensor> ppo_loss_bwd(
    torch::Tensor p, torch::Tensor lp, torch::Tensor coef, torch::Tensor h,
    torch::Tensor actions, torch::Tensor values, torch::Tensor vtarg,
    torch::Tensor gl, double vf_clip, double vf_coef, double ent_coef);
std::vector<torch::Tensor> vtrace_scan(
    torch::Tensor rewards, torch::Tensor dones, torch::Tensor values,
    torch::Tensor bootstrap, torch::Tensor rho, torch::Tensor c,
    double gamma);
std::vector<torch::Tensor> impala_loss_fwd(
    torch::Tensor logits, torch::Tensor values, torch::Tensor actions,
    torch::Tensor behaviour_logp, torch::Tensor rewards, torch::Tensor dones,
    torch::Tensor bootstrap, int64_t T, int64_t N, double gamma,
    double rho_clip, double pg_rho_clip, double c_clip, double vf_coeff,
    double ent_coeff, bool drop_last);
std::vector<torch::Tensor> impala_loss_bwd(
    torch::Tensor p, torch::Tensor lp, torch::Tensor h,
    torch::Tensor actions, torch::Tensor values, torch::Tensor vs,
    torch::Tensor pg_adv, torch::Tensor gl, int64_t T, int64_t N,
    double vf_coeff, double ent_coeff, bool drop_last);
int64_t dqn_nstep_ingest(
    torch::Tensor gfull, torch::Tensor model_ids, torch::Tensor actions,
    torch::Tensor rewards, torch::Tensor dones,
    std::vector<torch::Tensor> ring, int64_t T, int64_t N, int64_t capacity,
    int64_t written, int64_t n_step, double gamma);
std::vector<torch::Tensor> dqn_loss_fwd(
    torch::Tensor logits_s, torch::Tensor values_s, torch::Tensor logits_no,
    torch::Tensor values_no, torch::Tensor logits_nt, torch::Tensor values_nt,
    torch::Tensor actions, torch::Tensor ret, torch::Tensor disc,
    torch::Tensor has_next, double v_min, double v_max, bool dueling,
    bool double_q);
std::vector<torch::Tensor> dqn_loss_fwd_weighted(
    torch::Tensor logits_s, torch::Tensor values_s, torch::Tensor logits_no,
    torch::Tensor values_no, torch::Tensor logits_nt, torch::Tensor values_nt,
    torch::Tensor actions, torch::Tensor ret, torch::Tensor disc,
    torch::Tensor has_next, double v_min, double v_max, bool dueling,
    bool double_q, torch::Tensor weights);
std::vector<torch::Tensor> dqn_loss_bwd(
    torch::Tensor logits_s, torch::Tensor actions, torch::Tensor dq,
    torch::Tensor gl, bool dueling);
void per_ingest(torch::Tensor tree_sum, torch::Tensor tree_min,
                torch::Tensor max_prio, int64_t start, int64_t count,
                int64_t capacity, double alpha);
std::vector<torch::Tensor> per_sample(
    torch::Tensor tree_sum, torch::Tensor tree_min, torch::Tensor u,
    int64_t capacity, double beta);
void per_update(torch::Tensor tree_sum, torch::Tensor tree_min,
                torch::Tensor max_prio, torch::Tensor idx,
                torch::Tensor td_abs, int64_t capacity, double alpha,
                double eps);
void env_step_batch(std::vector<torch::Tensor> T, std::vector<double> fscal,
                    std::vector<int64_t> iscal);
void cached_step_fwd(std::vector<torch::Tensor> T, std::vector<double> fs);
void cached_step_bwd(std::vector<torch::Tensor> T, std::vector<double> fs,
                     bool defer_reduce);
bool cached_step_reduce_deferred(bool defer_reduce);
std::vector<int64_t> cached_step_fold_segments(std::vector<int64_t> offs);
void cached_step_fwd_staged(std::vector<torch::Tensor> T,
                            std::vector<double> fs,
                            std::vector<torch::Tensor> store,
                            torch::Tensor perm, torch::Tensor cursor,
                            torch::Tensor err,
                            std::vector<torch::Tensor> dims);
void cached_stage(std::vector<torch::Tensor> store,
                  std::vector<torch::Tensor> dst, torch::Tensor perm,
                  torch::Tensor cursor, torch::Tensor err,
                  std::vector<torch::Tensor> dims);
std::vector<torch::Tensor> lookahead_batch(
    torch::Tensor descs, torch::Tensor op_remaining, torch::Tensor op_worker,
    torch::Tensor op_priority, torch::Tensor out_indptr, torch::Tensor out_edges,
    torch::Tensor true_parent_count, torch::Tensor parent_done,
    torch::Tensor op_ready, torch::Tensor op_completed,
    torch::Tensor dep_remaining, torch::Tensor dep_is_flow,
    torch::Tensor dep_channel, torch::Tensor dep_priority, torch::Tensor dep_dst,
    torch::Tensor dep_ready, torch::Tensor dep_completed,
    torch::Tensor worker_best, torch::Tensor channel_best);
void actor_batch(torch::Tensor obs_gf, torch::Tensor obs_mask,
                 torch::Tensor obs_model, torch::Tensor obs_sched,
                 torch::Tensor done, torch::Tensor model_emb,
                 std::vector<torch::Tensor> head, torch::Tensor model_seq,
                 torch::Tensor sch_acc, int64_t mode, int64_t sip_ml_cap,
                 uint64_t seed, uint64_t step, torch::Tensor actions,
                 torch::Tensor gfull, torch::Tensor lp_all,
                 torch::Tensor logp, torch::Tensor value, torch::Tensor u);
void es_perturb(torch::Tensor theta, double sigma, uint64_t seed,
                uint64_t generation, torch::Tensor eps, torch::Tensor pop);
void es_update(torch::Tensor theta, torch::Tensor eps, torch::Tensor w,
               double scale, double decay, torch::Tensor out);
void actor_population(torch::Tensor obs_gf, torch::Tensor obs_mask,
                      torch::Tensor obs_model, torch::Tensor done,
                      torch::Tensor pop, torch::Tensor model_emb_pop,
                      std::vector<int64_t> head_offs, int64_t E, int64_t mode,
                      uint64_t seed, uint64_t step, torch::Tensor actions,
                      torch::Tensor lp_all, torch::Tensor logp,
                      torch::Tensor value, torch::Tensor u);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("row_mlp", &row_mlp, "fused LN+Linear+ReLU over rows");
    m.def("message_reduce", &message_reduce,
          "fused gather + LN + GEMV + ReLU + segment-mean message passing");
    m.def("segment_mean", &segment_mean, "per-graph mean of node embeddings");
    m.def("lookahead_batch", &lookahead_batch,
          "batched RAMP lookahead discrete-event simulation");
    m.def("message_reduce_train", &message_reduce_train,
          "message_reduce storing per-message activations for backward");
    m.def("message_reduce_bwd", &message_reduce_bwd,
          "fused MeanPool message-passing backward");
    m.def("row_mlp_bwd", &row_mlp_bwd, "fused LN+Linear+ReLU backward");
    m.def("row_mlp_mfma", &row_mlp_mfma,
          "LN+Linear+ReLU on v_mfma_f32_16x16x4_f32 tiles");
    m.def("message_mlp_mfma", &message_mlp_mfma,
          "per-message reduce-MLP on the matrix core");
    m.def("segment_combine", &segment_combine,
          "CSR segment mean of stored message activations");
    m.def("ppo_loss_fwd", &ppo_loss_fwd, "fused PPO clipped-surrogate loss");
    m.def("ppo_loss_bwd", &ppo_loss_bwd, "analytic PPO loss backward");
    m.def("vtrace_scan", &vtrace_scan,
          "V-trace recurrence over [T, N], bit-equal to vtrace_targets");
    m.def("impala_loss_fwd", &impala_loss_fwd,
          "fused IMPALA loss: row softmax, V-trace scan, ordered reduction");
    m.def("impala_loss_bwd", &impala_loss_bwd,
          "analytic IMPALA loss backward");
    m.def("dqn_nstep_ingest", &dqn_nstep_ingest,
          "n-step transitions of a [T, N] fragment written into the replay "
          "ring, bit-equal to nstep_transitions_reference");
    m.def("dqn_loss_fwd", &dqn_loss_fwd,
          "fused dueling double-DQN TD loss: row kernel, ordered reduction");
    m.def("dqn_loss_fwd_weighted", &dqn_loss_fwd_weighted,
          "importance-weighted DQN TD loss (prioritized replay); also "
          "returns the unweighted |td| per row");
    m.def("dqn_loss_bwd", &dqn_loss_bwd, "analytic DQN loss backward");
    m.def("per_ingest", &per_ingest,
          "prioritized replay: new slots enter the sum/min trees at "
          "max_prio^alpha");
    m.def("per_sample", &per_sample,
          "prioritized replay: sum-tree descent and importance weights");
    m.def("per_update", &per_update,
          "prioritized replay: new priorities for a minibatch's slots, "
          "last occurrence wins");
    m.def("segment_mean_bwd", &segment_mean_bwd,
          "per-graph mean backward (broadcast/scale)");
    m.def("flat_adam", &flat_adam,
          "fused grad-clip + Adam over flat param/grad/m/v buffers");
    m.def("message_reduce_bwd_mfma", &message_reduce_bwd_mfma,
          "matrix-core message-passing backward (3-stage MFMA)");
    m.def("flat_sumsq", &flat_sumsq, "capture-safe sum of squares");
    m.def("flat_sumsq_adam", &flat_sumsq_adam,
          "grad-norm partials + step count, then clip + Adam: the two-launch "
          "optimiser tail of the captured step");
    m.def("flat_sumsq_blocks", &flat_sumsq_blocks,
          "number of partial sums flat_sumsq_adam writes for numel floats");
    m.def("head_fwd", &head_fwd,
          "fused policy/value head forward (LN+graphMLP+concat+2 branches)");
    m.def("head_bwd", &head_bwd, "fused policy/value head backward");
    m.def("cached_step_fwd", &cached_step_fwd,
          "fully-fused cached-models PPO minibatch forward (GNN+head+loss)");
    m.def("cached_step_bwd", &cached_step_bwd,
          "analytic whole-net backward into the flat grad buffer; with "
          "defer_reduce the row jobs' partial sums stay in wg_scratch for "
          "flat_sumsq_adam_folded",
          pybind11::arg("T"), pybind11::arg("fs"),
          pybind11::arg("defer_reduce") = false);
    m.def("cached_step_reduce_deferred", &cached_step_reduce_deferred,
          "whether cached_step_bwd(defer_reduce) leaves the reduce to the "
          "tail under the current switches");
    m.def("cached_step_fold_segments", &cached_step_fold_segments,
          "the row jobs' (flat start, length, scratch offset) triples, then "
          "the split count and the split stride, from the host slot offsets");
    m.def("flat_sumsq_adam_folded", &flat_sumsq_adam_folded,
          "flat_sumsq_adam whose first launch also sums the row-split "
          "weight-grad partials into the flat gradient");
    m.def("cached_step_fwd_staged", &cached_step_fwd_staged,
          "cached_step_fwd whose first launch also gathers the minibatch "
          "from the device batch store (block 0 runs cached_stage's role)");
    m.def("cached_stage", &cached_stage,
          "gather one minibatch from the device batch store into the "
          "cached step's staged inputs; advances the device cursor");
    m.def("env_step_batch", &env_step_batch,
          "batched RAMP env step over vectorised envs (placement search + "
          "memo hash probe + event loop + obs encode)");
    m.def("actor_batch", &actor_batch,
          "device-side actors over vectorised envs: GNN policy head (greedy "
          "or Philox-sampled) and the six heuristic baselines, one launch");
    m.def("es_perturb", &es_perturb,
          "ES: Philox/Box-Muller noise eps [K,n] and the antithetic "
          "population pop [2K,n] = theta +- sigma * eps, one launch");
    m.def("es_update", &es_update,
          "ES: theta' = (theta + scale * sum_k w[k] eps[k]) - decay * theta");
    m.def("actor_population", &actor_population,
          "actor_batch's policy modes with the head weights and embedding "
          "table of row b taken from population member b / E, one launch");
}
