/* arbplf-mixture-deriv: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * The gradient of the site-aggregated log likelihood in the parameters of the rate mixture (no counterpart in the
 * reference; same filter as its run_json_script). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_mixture_deriv_string);
}
