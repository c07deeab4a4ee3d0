/* arbplf-spr: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * The log likelihood of subtree prune-and-regraft moves of the tree (no counterpart in the reference; same filter as its
 * run_json_script). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_spr_string);
}
