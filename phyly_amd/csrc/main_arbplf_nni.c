/* arbplf-nni: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * The log likelihood of nearest-neighbour interchanges of the tree (no counterpart in the reference; same filter as its
 * run_json_script). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_nni_string);
}
