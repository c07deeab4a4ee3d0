/* arbplf-place: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * The log likelihood of the tree with new taxa attached to its edges (no counterpart in the reference; same filter as its
 * run_json_script). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_place_string);
}
