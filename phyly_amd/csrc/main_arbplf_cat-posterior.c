/* arbplf-cat-posterior: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * The posterior probability of each rate category at each site (no counterpart in the reference; same filter as its run_json_script). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_cat_posterior_string);
}
