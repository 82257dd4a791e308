// sigp_loo_grad_ard_batch: the leave-one-out scores AND the exact derivatives of one of them with respect to (log l_1 .. log l_d, log sn~) for
// lockstep groups of fits on the data sets resident after sigp_batch_upload (include/sigp.h): sigp_nlml_grad_ard_batch's staging and group
// fit, sigp_loo_grad_batch's scores, and sigp_loo_grad_ard's gradient with the member on a grid axis (looard.hpp, ardgrad.hpp).  Included
// inside extern "C" of sigp.hip, after sigp_ardbatch.inc (the staging) and sigp_looard.inc (loo_ard_pass_members).
//
// Per group of nb members, on slot 0:
//   staging              ard_stage_group: every member's scaled features, ride rows and y ("data set b" of the staging area), sn~ in ArdStage::sn
//   fit                  batch_group_fit_on at ell = 1 on the staging pointers, no ride points
//   scores               loo_launch with nb members (U = L~^-T in gU; q = y^T A~ in the slot's result rows), as sigp_loo_grad_batch calls it
// and for a gradient, every step for all members at once:
//   P = U U^T            kinv_lower into gK;  a = U z (alpha_from_U) into the member's vectors;  mirror_P
//   beta, gamma, eps     loo_ard_coef_kernel, one block per member;  v = P beta and P Gamma into gD: loo_ard_scale_kernel
//   M = (P Gamma) P^T    syrk_set on the lower tile space into gU, which is dead by then (n^3 flops per member, whatever d)
//   the ARD pass         loo_ard_pass_members: the tile pass on the staged features, the fixed-order sums, ONE copy of the group's gradients
// then batch_scores_fetch, sync_slot, batch_scores_scatter.  A member whose exp(theta) is not finite and positive rides along at harmless
// parameters (the ok[] of sigp_nlml_grad_ard_batch); it and a member whose K~ is not SPD get +inf in both scores and every gradient entry
// and what batch_scores_scatter leaves a failed member in mean / var.  Members share no memory: their group mates keep their bits.
// Memory beside the slot: gU, gK, gD [G][n_pad][n_pad] as sigp_loo_grad_batch, the staging area, the centred features, LooArdGroupVecs and
// LooArdGroupParts (score_layout.hpp).  Profile classes: the staging SIGP_KC_KBUILD, the gradient's work SIGP_KC_MLII (sigp_loo_grad_ard's
// entries, their figures times nb).
// Out of scope: sigp_small_*, the fp32 engine, sharded fits.  The leave-block-out scores in groups: sigp_cv_grad_ard_batch.
// The driver is ard_score_batch (sigp_cvardbatch.inc), which the two entries share: the leave-block-out form differs in the score's launches
// (cv_launch with the adjoint) and in the steps up to M (cv_ard_products), so it is defined behind sigp_cvard.inc; cv = NULL runs the steps above.

struct CvFolds { int64_t block, gap; };
static int ard_score_batch(sigp_handle* h, const char* what, const CvFolds* cv, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta,
                           int64_t ldtheta, int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad);

int sigp_loo_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta, int sigma_mode,
                            int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad) {
  return ard_score_batch(h, "loo_grad_ard_batch", nullptr, first, count, kernel_id, theta, ntheta, ldtheta, sigma_mode, criterion, mean, var, nstride, score, grad, ldgrad);
}
